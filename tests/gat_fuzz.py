"""The randomised battery of the GAT family, shared by test_gat_fuzz_host.py (no GPU), test_gat_fuzz.py (GPU) and
tools/soak_fuzz.py --gat: the draw of one case from a seed, the case's graph and inputs, its float64 reference, the
kernels its launch profile must show, its bounds, and the call on the device.  The module imports without a GPU.

draw(seed) depends on nothing but the seed: the family is FAMILIES[seed % 6], everything else comes from
np.random.RandomState(BASE + seed), every draw made whichever branch uses it, so a case keeps its graph when a branch
changes.  BASE = 36088 came out of a search over bases for one at which seeds 0..47 meet every coverage condition of
test_gat_fuzz_host.py::test_coverage_of_the_suite_seeds (about one base in ten thousand does); the conditions are
asserted there, none was relaxed to fit a base.

No reference arithmetic is new.  The expected values are gat_reference.gat_scores / gat_layer,
gatv2_reference.gatv2_scores / gatv2_datt_scale, test_gat_launch_geometry.masked_gat_layer_one_head with
dropout_reference.multipliers, fused_gatv2_reference.reference and gatv2_dropout_reference.reference, in float64, one head
at a time (no float64 temporary exceeds (E, d) values).  reference(..., dtype=torch.float32) is the same code in fp32:
the "plain torch" evaluation the host tier holds to half of every bound.

Cases with (seed // 6) % 4 == 3 are the large stratum: profile_graph at chunk_size 1, sized from the CU count so that
both backward passes run at 2 or 3 chunks per lane group (the score forwards at min(that, sddmm_cpg)); always fp32, a
fast shape with h * d <= 128, aligned, spmm_cpg at its default or 16.
Its output gradient is standard normal / 8 (LARGE_GRAD_SCALE): with shuffled chunk lists a row of 5000 slots is summed by
2500 fp32 atomic adds, whose rounding alone (about 1.4e-5 at unit scale on an element that cancels to below 1) moved dxl of
seed 19 between 0.42 and 1.23 of its bound over five runs on an MI355X; every gradient is linear in the output gradient, so
the same kernels then sit near a tenth of the bound, and the bound stays what it is.

Two places where the mirrored dispatch rules decide, not the draw: GATScores has fast kernels for h = 16 (gat.hip), so of
the "generic" head counts {3, 16} only 3 is generic by shape; and its tables need the alignment of one item, min(4 h, 16)
bytes, so a table 4 bytes off leaves h = 1 on the fast kernels.
The autograd entry of the two score families is GATScores / GATv2Scores.apply followed by backward(dy): the composed
*_attention_step helpers end in VectorSPMM, whose output has the row count of its value table, so they cannot run on the
rectangular graphs the battery draws (test_gat_fuzz.py replays all six step helpers from a HIP graph)."""
import dataclasses
import functools
import os
import sys

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:       # (imported outside pytest, by tools/soak_fuzz.py or from tests/ by hand)
    sys.path.insert(0, _ROOT)

import dropout_reference as DR
import fused_gatv2_reference as R
import gatv2_dropout_reference as RD
from gat_reference import gat_layer, gat_scores
from gatv2_reference import gatv2_datt_scale, gatv2_scores
from test_gat_launch_geometry import (DROP_FAST, FUSED_FAST, GAT_FAST, GATV2_FAST, _cpg, _fused_inputs, _gat_G,
                                      _gat_inputs, _generic, _groups_wanted, _shifted, masked_gat_layer_one_head,
                                      profile_graph, reorder_chunks_vectorised)
from util import random_graph

BASE = 36088
N_SUITE = 48
FAMILIES = ("gat_scores", "gatv2_scores", "fused_gat", "fused_gat_dropout", "fused_gatv2", "fused_gatv2_dropout")
GATV2_FAMILIES = ("gatv2_scores", "fused_gatv2", "fused_gatv2_dropout")
DROPOUT_FAMILIES = ("fused_gat_dropout", "fused_gatv2_dropout")
BINDINGS = ("ctypes", "cpp_ext", "torch_ops")
GAT_FAST_H = (1, 2, 4, 8, 16)                       # GO_DISPATCH_GAT_H (gat.hip)
GAT_OTHER_H = (3, 16)
GENERIC_HD = ((3, 5), (1, 8), (2, 16), (1, 128), (6, 16))
LARGE_GRAD_SCALE = 0.125
LARGE_HD = tuple(hd for hd in R.FAST if hd[0] * hd[1] <= 128)
GV2_FAST = {"gv2attn_fwd": "k_gv2attn_fwd_f32", "gv2attn_pack": "k_gv2attn_pack_f32",
            "gv2attn_bwd_row": "k_gv2attn_bwd_row_f32", "gv2attn_bwd_col": "k_gv2attn_bwd_col_f32",
            "gv2attn_datt_fin": "k_gv2attn_datt_fin_f32"}
GV2_DROP_FAST = {"gv2attn_drop_fwd": "k_gv2attn_drop_fwd_f32", "gv2attn_pack": "k_gv2attn_pack_f32",
                 "gv2attn_drop_bwd_row": "k_gv2attn_drop_bwd_row_f32",
                 "gv2attn_drop_bwd_col": "k_gv2attn_drop_bwd_col_f32", "gv2attn_datt_fin": "k_gv2attn_datt_fin_f32"}
TAG_PREFIX = {"gat_scores": ("gat_fwd", "gat_bwd_"), "gatv2_scores": ("gatv2_",), "fused_gat": ("gat_attn_",),
              "fused_gat_dropout": ("gat_attn_",), "fused_gatv2": ("gv2attn_",), "fused_gatv2_dropout": ("gv2attn_",)}
OUTPUTS = {"gat_scores": ("y", "del", "der"), "gatv2_scores": ("y", "dxl", "dxr", "datt"),
           "fused_gat": ("o", "del", "der", "dV"), "fused_gat_dropout": ("o", "del", "der", "dV"),
           "fused_gatv2": ("o", "stats", "dxl", "dxr", "datt"), "fused_gatv2_dropout": ("o", "stats", "dxl", "dxr", "datt")}


@dataclasses.dataclass(frozen=True)
class Case:
    seed: int
    family: str
    h: int
    d: int                  # 0 for gat_scores, which has no feature axis
    dtype: str              # "float32" or "float64"
    large: bool
    target_cpg: int         # large stratum: chunks per lane group of both backward passes; else 0
    n_src: int
    n_dst: int
    n_edges: int            # before zero_rows and hub (small stratum)
    chunk_size: int
    zero_rows: float
    hub: int
    graph_seed: int
    shuffled: bool          # the chunk lists of both orientations in random order
    slope: float
    kind: str               # "normal" or "ties" (fused_gatv2_reference.inputs)
    p: float                # dropout families only, else 0
    philox_seed: int
    offset: int
    spmm_cpg: int           # 0: the default stays
    sddmm_cpg: int          # 0: the default stays
    force_generic: bool
    misaligned: int         # index of the input table that sits one element (4 bytes in fp32) off a 16-byte boundary, or -1
    entry: str              # one of BINDINGS (raw forward and backward ops) or "autograd"
    grad_view: str          # autograd entry: "contiguous", "expand" (stride 0) or "transposed"
    input_seed: int

    @property
    def torch_dtype(self):
        return getattr(torch, self.dtype)

    @property
    def dropped(self):
        return self.family in DROPOUT_FAMILIES and self.p > 0

    @property
    def group(self):
        """lanes of a lane group of the family's fast gather passes"""
        return _gat_G(self.h) if self.family == "gat_scores" else 16


def draw(seed):
    seed = int(seed)
    family = FAMILIES[seed % 6]
    rng = np.random.RandomState(BASE + seed)
    large = (seed // 6) % 4 == 3
    pick = lambda xs: xs[int(rng.randint(len(xs)))]
    fast_shape = bool(rng.rand() < 0.7)
    fast_h, other_h = pick(GAT_FAST_H), pick(GAT_OTHER_H)
    fast_hd, other_hd, large_hd = pick(R.FAST), pick(GENERIC_HD), pick(LARGE_HD)
    if family == "gat_scores":
        h, d = (fast_h if fast_shape or large else other_h), 0
    else:
        h, d = large_hd if large else (fast_hd if fast_shape else other_hd)
    fp64 = bool(rng.rand() < 0.15) and not large
    n_src = int(rng.randint(40, 700))
    n_other = int(rng.randint(40, 700))
    n_dst = n_src if rng.rand() < 0.5 else n_other
    n_edges = int(rng.randint(1, 40)) * n_src
    chunk_size, zero_rows, hub = pick((1, 3, 7, 32, 64)), pick((0.0, 0.2)), pick((0, 0, 300, 1500))
    target_cpg, graph_seed = pick((2, 3)), int(rng.randint(1 << 30))
    shuffled = bool(rng.rand() < 0.3)
    slope = pick((0.2, 0.2, 0.0, -0.1, 1.0))
    ties = bool(rng.rand() < 0.1) and family in GATV2_FAMILIES
    p = pick((0.1, 0.5, 0.9))
    p = 0.0 if rng.rand() < 0.1 else p
    small_seed, big_seed = int(rng.randint(0, 2 ** 32, dtype=np.int64)), int(rng.randint(2 ** 32, 2 ** 63, dtype=np.int64))
    philox_seed = small_seed if rng.rand() < 0.5 else big_seed
    offset = pick((0, 1, 2 ** 32 - 1))
    spmm_cpg, sddmm_cpg = pick((0, 1, 2, 16)), pick((0, 1, 3, 8))
    force_generic = bool(rng.rand() < 0.15) and not large
    table = int(rng.randint(3))
    misaligned = table % (2 if family == "gat_scores" else 3) if rng.rand() < 0.1 and not large else -1
    binding = pick(BINDINGS)
    entry = binding if rng.rand() < 0.5 else "autograd"
    view = pick(("expand", "transposed"))
    grad_view = view if rng.rand() < 0.15 and entry == "autograd" else "contiguous"
    input_seed = int(rng.randint(1 << 30))
    drop = family in DROPOUT_FAMILIES
    return Case(seed=seed, family=family, h=int(h), d=int(d), dtype="float64" if fp64 else "float32", large=large,
                target_cpg=int(target_cpg) if large else 0, n_src=n_src, n_dst=n_dst, n_edges=n_edges,
                chunk_size=1 if large else int(chunk_size), zero_rows=0.0 if large else float(zero_rows),
                hub=0 if large else int(hub), graph_seed=graph_seed, shuffled=shuffled, slope=float(slope),
                kind="ties" if ties else "normal", p=float(p) if drop else 0.0, philox_seed=philox_seed if drop else 0,
                offset=int(offset) if drop else 0, spmm_cpg=int(spmm_cpg) if not large else (0, 16)[spmm_cpg % 2],
                sddmm_cpg=int(sddmm_cpg), force_generic=force_generic, misaligned=int(misaligned), entry=entry,
                grad_view=grad_view, input_seed=input_seed)


# ---- the dispatch rules, mirrored ---------------------------------------------------------------------------------
def fast_shape(case):
    """the shape has fp32 fast kernels (gat.hip, gatv2.hip, gat_attention.hip, gatv2_attention.hip)"""
    return case.h in GAT_FAST_H if case.family == "gat_scores" else (case.h, case.d) in R.FAST


def _table_breaks_alignment(case):
    if case.misaligned < 0:
        return False
    if case.family == "gat_scores":                  # gat_aligned: one item of min(4 h, 16) bytes
        return 4 % min(4 * case.h, 16) != 0
    return True                                      # every other family asks 16 bytes of each table


def expected_kernels(case):
    """{profile tag: kernel name} of one forward and backward.  Every op of the battery is called with the plans of
    both orientations; the drawn misaligned table is an input that every pass reads."""
    ok = case.dtype == "float32" and not case.force_generic and fast_shape(case) and not _table_breaks_alignment(case)
    fam = case.family
    if fam == "gat_scores":
        return dict(GAT_FAST) if ok else _generic(GAT_FAST)
    if fam == "gatv2_scores":
        return dict(GATV2_FAST) if ok else _generic(GATV2_FAST)
    if fam in ("fused_gat", "fused_gat_dropout"):
        names = DROP_FAST if case.dropped else FUSED_FAST
        if not ok:
            return _generic(names)
        return _generic(names, "gat_attn_stats") if case.shuffled else dict(names)     # the stats need a row_owned plan
    names = GV2_DROP_FAST if case.dropped else GV2_FAST
    fwd = "gv2attn_drop_fwd" if case.dropped else "gv2attn_fwd"
    if not ok:       # the generic row pass adds datt by atomics: no datt_fin
        return {t: "k_%s_generic" % t for t in names if t != "gv2attn_datt_fin"}
    return dict(names, **{fwd: "k_%s_generic" % fwd}) if case.shuffled else dict(names)  # the forward needs row_owned


def all_fast(case):
    return all(k.endswith("_f32") for k in expected_kernels(case).values())


def bounds(case):
    """(dict(rtol, atol), K): the bounds of the family's own test module; datt within K * S"""
    if case.dtype == "float64":
        return dict(R.TOL64), R.K64
    return dict(rtol=1e-4, atol=1e-5 / (1 - case.p)), R.K32


# ---- graph and inputs ------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Built:
    g: object               # the AttnGraph on the CPU (src, dst in row-major order: what the references take)
    csr: tuple              # the eight index arrays the ops get (chunk lists shuffled or not), on the CPU
    inputs: tuple           # the family's tables in case.dtype, on the CPU
    grad: torch.Tensor      # dy (score families) or dO, contiguous, with the values of case.grad_view


def _view_values(t, view):
    """the values a gradient handed over as `view` holds (an expand is constant along its stride-0 axis)"""
    if view != "expand":
        return t
    return (t[:1] if t.dim() == 1 else t[..., :1]).expand_as(t).contiguous()


def as_view(t, view):
    """t's values as the non-contiguous tensor autograd would hand over"""
    if view == "expand":
        v = (t[:1] if t.dim() == 1 else t[..., :1]).expand_as(t)
    elif view == "transposed":
        v = torch.stack([t, t], 1)[:, 0] if t.dim() == 1 else t.transpose(0, -1).contiguous().transpose(0, -1)
    else:
        return t
    assert not v.is_contiguous() and torch.equal(v, t)
    return v


def drawn_graph(case, n_cu):
    """The graph of a case (of this battery or of gat_edge_fuzz): large stratum sized for n_cu compute units."""
    if case.large:
        g = profile_graph(int((case.target_cpg + 0.5) * _groups_wanted(n_cu, case.group)), seed=case.graph_seed)
        for C in (g.n_row_chunks, g.n_col_chunks):
            assert _cpg(C, n_cu, case.group, 16) == case.target_cpg and C % case.target_cpg != 0, (case, C)
        return g
    return random_graph(case.n_src, case.n_dst, case.n_edges, seed=case.graph_seed, chunk_size=case.chunk_size,
                        zero_rows=case.zero_rows, hub=case.hub or None)


def chunk_lists(case, g):
    """The eight index arrays the ops get: g's, with the chunk lists of both orientations in random order if drawn so."""
    if not case.shuffled:
        return g.csr_args()
    gen = torch.Generator().manual_seed(case.input_seed)
    pr = reorder_chunks_vectorised(g.ptr_r, g.row, g.eid_r, g.indices_r, torch.randperm(g.n_row_chunks, generator=gen))
    pc = reorder_chunks_vectorised(g.ptr_c, g.col, g.eid_c, g.indices_c, torch.randperm(g.n_col_chunks, generator=gen))
    return (pr[1], pr[0], pr[2], pr[3], pc[1], pc[0], pc[2], pc[3])


def build(case, n_cu):
    """The case's graph (large stratum: sized for n_cu compute units) and inputs."""
    g = drawn_graph(case, n_cu)
    csr = chunk_lists(case, g)
    dt = case.torch_dtype
    if case.family == "gat_scores":
        *tables, grad = _gat_inputs(g, case.h, case.input_seed)
    elif case.family in ("fused_gat", "fused_gat_dropout"):
        *tables, grad = _fused_inputs(g, case.h, case.d, case.input_seed)
    else:
        *tables, grad = R.inputs(g, case.h, case.d, case.input_seed, dt, case.kind, case.slope)
        if case.family == "gatv2_scores":
            gen = torch.Generator().manual_seed(case.input_seed + 1)
            grad = torch.randn((g.n_edges,) if case.h == 1 else (g.n_edges, case.h), generator=gen, dtype=dt)
    if case.large:
        grad = grad * LARGE_GRAD_SCALE
    return Built(g, csr, tuple(t.to(dt) for t in tables), _view_values(grad.to(dt), case.grad_view))


# ---- the references, one head at a time ------------------------------------------------------------------------------
def _per_head(like, node_dims):
    """[(select head k)], join of per-head node tensors, join of per-head parameter tensors"""
    if like.dim() == node_dims:
        return [lambda x: x], (lambda xs: xs[0]), (lambda xs: xs[0])
    return ([(lambda x, k=k: x[:, k]) for k in range(like.size(1))], (lambda xs: torch.stack(xs, 1)),
            (lambda xs: torch.stack(xs, 0)))


def reference(case, built, dtype=torch.float64):
    """{output name: expected tensor} (and "S", the scale of datt's bound, always from float64) by autograd in `dtype`"""
    g, x, grad, slope = built.g, built.inputs, built.grad, case.slope
    fam = case.family
    if fam == "gat_scores":
        r = [t.to(dtype).clone().requires_grad_(True) for t in x]
        y = gat_scores(g.src, g.dst, r[0], r[1], slope)
        y.backward(grad.to(dtype))
        return {"y": y.detach(), "del": r[0].grad, "der": r[1].grad}
    if fam == "gatv2_scores":
        xl, xr, att = x
        sel, join, stack0 = _per_head(xl, 2)
        outs = [[] for _ in range(5)]
        for k, head in enumerate(sel):
            att_k, dy_k = (att, grad) if xl.dim() == 2 else (att[k], grad[:, k])
            r = [t.to(dtype).clone().requires_grad_(True) for t in (head(xl), head(xr), att_k)]
            y = gatv2_scores(g.src, g.dst, r[0], r[1], r[2], slope)
            y.backward(dy_k.to(dtype))
            S = gatv2_datt_scale(g.src, g.dst, head(xl), head(xr), dy_k, slope)
            for lst, t in zip(outs, (y.detach(), r[0].grad, r[1].grad, r[2].grad, S)):
                lst.append(t)
        return {"y": join(outs[0]), "dxl": join(outs[1]), "dxr": join(outs[2]), "datt": stack0(outs[3]),
                "S": stack0(outs[4])}
    if fam in ("fused_gat", "fused_gat_dropout"):
        el, er, V = x
        sel, join, _ = _per_head(el, 1)
        mult = DR.multipliers(g.src.numpy(), g.dst.numpy(), len(sel), case.p, case.philox_seed, case.offset,
                              dtype) if case.dropped else None
        outs = [[] for _ in range(4)]
        for k, head in enumerate(sel):
            r = [head(t).to(dtype).clone().requires_grad_(True) for t in x]
            if mult is None:
                o = gat_layer(g.src, g.dst, g.n_src, r[0], r[1], r[2], slope)
            else:
                o = masked_gat_layer_one_head(g.src, g.dst, g.n_src, r[0], r[1], r[2], slope, mult[:, k])
            o.backward(head(grad).to(dtype))
            for lst, t in zip(outs, (o.detach(), r[0].grad, r[1].grad, r[2].grad)):
                lst.append(t)
        return dict(zip(OUTPUTS[fam], (join(ts) for ts in outs)))
    if case.dropped:
        ref = RD.reference(g, *x, grad, slope, case.p, case.philox_seed, case.offset, dtype)
    else:
        ref = R.reference(g, *x, grad, slope, dtype)
    return dict(zip(OUTPUTS[fam] + ("S",), ref[:6]))


def ratios(case, got, want):
    """{output name: used fraction of its bound}, datt as max |err| / (K * S)"""
    tol, K = bounds(case)
    out = {}
    for name in OUTPUTS[case.family]:
        if name not in got:
            continue
        if name == "datt":
            out[name] = R.datt_ratio(got[name], want[name], want["S"]) / K
        else:
            out[name] = R.ratio(got[name], want[name], tol)
    return out


@functools.lru_cache(maxsize=None)
def case_data(seed, n_cu):
    """(case, built, float64 reference) of a seed, computed once per process and left unchanged"""
    case = draw(seed)
    built = build(case, n_cu)
    return case, built, reference(case, built)


# ---- the call on the device ---------------------------------------------------------------------------------------
class _Csr:
    """what the functions.*_step helpers read of a graph: its eight index arrays"""
    def __init__(self, csr):
        self.csr = tuple(csr)
        self.row, self.ptr_r, self.eid_r, self.indices_r = self.csr[:4]

    def csr_args(self):
        return self.csr


def set_knobs(case):
    from custom_op_benchmark_amd import _lib
    if case.spmm_cpg:
        _lib.tune("spmm_cpg", case.spmm_cpg)
    if case.sddmm_cpg:
        _lib.tune("sddmm_cpg", case.sddmm_cpg)
    if case.force_generic:
        _lib.tune("force_generic", 1)


def assert_cpg(case, built, n_cu, sddmm_cpg, spmm_cpg):
    """Large stratum, as test_gat_launch_geometry._assert_cpg: the mirrored cpg of both backward orientations is the drawn
    one with a clipped last group; the score forwards run at min(that, sddmm_cpg)."""
    for name, C in (("row-major", built.g.n_row_chunks), ("column-major", built.g.n_col_chunks)):
        got = _cpg(C, n_cu, case.group, spmm_cpg)
        assert got == case.target_cpg, ("the %s pass of %s runs at cpg = %d, not %d: %d chunks on %d CUs, G = %d, "
                                        "spmm_cpg = %d" % (name, case, got, case.target_cpg, C, n_cu, case.group,
                                                           spmm_cpg))
        assert C % got != 0, "%s: %d chunks are a multiple of cpg = %d" % (name, C, got)
    if case.family in ("gat_scores", "gatv2_scores"):
        fwd = _cpg(built.g.n_row_chunks, n_cu, case.group, sddmm_cpg)
        assert fwd == min(case.target_cpg, sddmm_cpg), (case, fwd)
    return case.target_cpg


def off_boundary(t):
    """t's values in a view that starts one element into its storage: 4 bytes off a 16-byte boundary in fp32 (_shifted),
    8 bytes off in fp64 (the generic kernels whatever the alignment)"""
    if t.element_size() == 4:
        return _shifted(t)
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


def run(case, built, dev):
    """One forward and backward of the case on `dev` through its drawn entry -> {output name: tensor}"""
    from custom_op_benchmark_amd import functions, graphop as ops
    a8 = tuple(t.to(dev) for t in built.csr)
    x = [t.to(dev) for t in built.inputs]
    if case.misaligned >= 0:
        x[case.misaligned] = off_boundary(x[case.misaligned])
    grad = built.grad.to(dev)
    fam, slope = case.family, case.slope
    drop = (case.p, case.philox_seed, case.offset) if fam in DROPOUT_FAMILIES else ()
    names = OUTPUTS[fam]
    if case.entry == "autograd":
        leaves = [t.requires_grad_(True) for t in x]
        gv = as_view(grad, case.grad_view)
        if fam == "gat_scores":
            out = functions.GATScores.apply(*a8, *leaves, slope)
            out.backward(gv)
        elif fam == "gatv2_scores":
            out = functions.GATv2Scores.apply(*a8, *leaves, slope)
            out.backward(gv)
        else:
            step = {"fused_gat": functions.fused_gat_attention_step,
                    "fused_gat_dropout": functions.fused_gat_attention_dropout_step,
                    "fused_gatv2": functions.fused_gatv2_attention_step,
                    "fused_gatv2_dropout": functions.fused_gatv2_attention_dropout_step}[fam]
            out = step(_Csr(a8), *leaves, gv, *drop, slope)
        grads = [t.grad for t in leaves]
        return dict(zip([n for n in names if n != "stats"], [out.detach()] + grads))
    m = {"ctypes": ops, "cpp_ext": ops.cpp_ext if ops.cpp_ext is not None else ops, "torch_ops": torch.ops.graphop}[
        case.entry]
    if fam == "gat_scores":
        return dict(zip(names, [m.gat_scores_forward(*a8[:4], *x, slope)] + list(m.gat_scores_backward(*a8, *x, grad, slope))))
    if fam == "gatv2_scores":
        return dict(zip(names, [m.gatv2_scores_forward(*a8[:4], *x, slope)]
                        + list(m.gatv2_scores_backward(*a8, *x, grad, slope))))
    op = {"fused_gat": "gat_attention", "fused_gat_dropout": "gat_attention_dropout", "fused_gatv2": "gatv2_attention",
          "fused_gatv2_dropout": "gatv2_attention_dropout"}[fam]
    o, stats = getattr(m, op + "_forward")(*a8[:4], *x, slope, *drop)
    grads = list(getattr(m, op + "_backward")(*a8, *x, o, stats, grad, slope, *drop))
    out = dict(zip([n for n in names if n != "stats"], [o] + grads))
    out["stats"] = stats
    return out
