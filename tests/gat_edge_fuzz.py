"""The randomised battery of the fused GAT layer with an edge term (graphop.gat_edge_attention_forward / _backward,
functions.FusedGATEdgeAttention), shared by test_gat_edge_fuzz_host.py (no GPU), test_gat_edge_fuzz.py (GPU) and
tools/soak_fuzz.py --gat-edge.  The structure, the graph draw, the views and the device helpers are those of gat_fuzz.py
(imported, not restated); this module adds what exists only with the edge term: the ee kind, the edge numbering, need_dee
and the alignment rule of ee.  The module imports without a GPU.

draw(seed) depends on nothing but the seed: everything comes from np.random.RandomState(BASE + seed), every draw made
whichever branch uses it.  Seeds with seed % 4 == 3 are the large stratum (gat_fuzz.py: profile_graph at chunk_size 1,
sized from the CU count so that both backward passes run at 2 or 3 chunks per lane group with a clipped last group; fp32,
a fast shape with h * d <= 128, aligned, output gradient * gat_fuzz.LARGE_GRAD_SCALE for the reason written there).
BASE = 316 came out of a search over bases 0, 1, 2, ... for the first at which seeds 0..23 meet every coverage condition
of test_gat_edge_fuzz_host.py::test_coverage_of_the_suite_seeds (five of the first 325 do, neighbours of one another,
since neighbouring bases share 23 of their 24 generators); the conditions are asserted there, none was relaxed to fit a
base.

The output gradient of the "ties" kind is standard normal / 2 (TIES_GRAD_SCALE).  Its scores are sums of three integers
in [-3, 3], twice as spread as the unit kind's, so the softmax is sharp, single terms of del's row sum reach |da| ~
sqrt(d), and at slope 0 the sum of the positive-side terms cancels to near zero: torch's own fp32 evaluation of seed 10
((1, 64), slope 0, 27 slots a row) used 0.56 of del's bound with a unit gradient, over the half the host tier allows a
reference.  Every gradient is linear in the output gradient and z == 0 does not depend on it, so the same case then uses
0.32, and the bound stays what it is.

The edge numbering: "row_identity" keeps eid_r == arange(E) (the row-major passes get a NULL eid), "permuted" renumbers
the edges at random (gat_edge_reference.permute_edge_ids), "col_identity" numbers them in column-major slot order
(gat_edge_reference.column_identity_edge_ids): eid_c == arange(E), the COLUMN-major pass gets a NULL eid and the
row-major ids are a non-trivial permutation.  Shuffled chunk lists move the slots, so their plans never say eid_identity.

No reference arithmetic is new: the expected values are gat_edge_reference.gat_edge_layer with
dropout_reference.multipliers, by autograd in float64, one head at a time (no float64 temporary exceeds (E, d) values);
reference(..., dtype=torch.float32) is the same code in fp32, which the host tier holds to half of every bound.  The
bounds are gat_edge_reference.TOL32 with atol / (1 - p) (as gat_fuzz.bounds) and TOL64."""
import dataclasses
import functools

import numpy as np
import torch

import gat_fuzz as F
import dropout_reference as DR
import gat_edge_reference as E
from gat_fuzz import Built, _Csr, as_view, off_boundary

BASE = 316
N_SUITE = 24
FAST_HD = tuple(F.R.FAST)
KINDS = ("unit", "ties", "large", "zero")
NUMBERINGS = ("permuted", "row_identity", "col_identity")
TABLES = ("el", "er", "ee", "V")
ENTRIES = F.BINDINGS + ("autograd",)
OUTPUTS = E.NAMES                                     # o, del, der, dee, dV (and "stats" from the raw entries)
TAG_PREFIX = "gat_edge_attn_"
TIES_GRAD_SCALE = 0.5


@dataclasses.dataclass(frozen=True)
class Case:
    seed: int
    h: int
    d: int
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
    kind: str               # one of KINDS (gat_edge_reference.inputs)
    numbering: str          # one of NUMBERINGS
    p: float
    philox_seed: int
    offset: int
    need_dee: bool
    spmm_cpg: int           # 0: the default stays
    sddmm_cpg: int          # 0: the default stays
    force_generic: bool
    misaligned: int         # index into TABLES of the input that sits one element off a 16-byte boundary, or -1
    entry: str              # one of ENTRIES
    grad_view: str          # autograd entry: "contiguous", "expand" (stride 0) or "transposed"
    input_seed: int

    family = "fused_gat_edge"
    group = 16              # lanes of a lane group of the fast gather passes

    @property
    def torch_dtype(self):
        return getattr(torch, self.dtype)

    @property
    def dropped(self):
        return self.p > 0


def draw(seed):
    seed = int(seed)
    rng = np.random.RandomState(BASE + seed)
    large = seed % 4 == 3
    pick = lambda xs: xs[int(rng.randint(len(xs)))]
    fast_shape = bool(rng.rand() < 0.7)
    fast_hd, other_hd, large_hd = pick(FAST_HD), pick(F.GENERIC_HD), pick(F.LARGE_HD)
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
    kind, numbering = pick(KINDS), pick(NUMBERINGS)
    p = pick((0.0, 0.1, 0.5, 0.9))
    small_seed, big_seed = int(rng.randint(0, 2 ** 32, dtype=np.int64)), int(rng.randint(2 ** 32, 2 ** 63, dtype=np.int64))
    philox_seed = small_seed if rng.rand() < 0.5 else big_seed
    offset = pick((0, 1, 2 ** 32 - 1))
    need_dee = bool(rng.rand() < 0.6)
    spmm_cpg, sddmm_cpg = pick((0, 1, 2, 16)), pick((0, 1, 3, 8))
    force_generic = bool(rng.rand() < 0.1) and not large
    table = int(rng.randint(len(TABLES)))
    misaligned = table if rng.rand() < 0.3 and not large else -1
    binding = pick(F.BINDINGS)
    entry = binding if rng.rand() < 0.6 else "autograd"
    view = pick(("expand", "transposed"))
    grad_view = view if rng.rand() < 0.5 and entry == "autograd" else "contiguous"
    input_seed = int(rng.randint(1 << 30))
    return Case(seed=seed, h=int(h), d=int(d), dtype="float64" if fp64 else "float32", large=large,
                target_cpg=int(target_cpg) if large else 0, n_src=n_src, n_dst=n_dst, n_edges=n_edges,
                chunk_size=1 if large else int(chunk_size), zero_rows=0.0 if large else float(zero_rows),
                hub=0 if large else int(hub), graph_seed=graph_seed, shuffled=shuffled, slope=float(slope), kind=kind,
                numbering=numbering, p=float(p), philox_seed=philox_seed if p > 0 else 0,
                offset=int(offset) if p > 0 else 0, need_dee=need_dee,
                spmm_cpg=int(spmm_cpg) if not large else (0, 16)[spmm_cpg % 2], sddmm_cpg=int(sddmm_cpg),
                force_generic=force_generic, misaligned=int(misaligned), entry=entry, grad_view=grad_view,
                input_seed=input_seed)


# ---- the dispatch rules of host_gat_attn_ops.h, mirrored -----------------------------------------------------------------
def fast_shape(case):
    return (case.h, case.d) in FAST_HD


def tables_aligned(case):
    """el, er and V need 16 bytes; ee its item width, 4 * min(h, 4) bytes (gat_aligned).  The drawn table sits one
    element off: 4 bytes in fp32 (8 in fp64, where nothing is fast anyway)."""
    if case.misaligned < 0:
        return True
    if TABLES[case.misaligned] != "ee":
        return False
    return 4 % (4 * min(case.h, 4)) == 0


def expected_kernels(case):
    """{profile tag: kernel name} of one forward and backward, called with the plans of both orientations: exactly
    five tags.  p == 0 runs under the undropped tags; the pack kernel is the plain layer's (P holds no edge term)."""
    ok = case.dtype == "float32" and not case.force_generic and fast_shape(case) and tables_aligned(case)
    drop = "drop_" if case.dropped else ""
    sfx = lambda fast: "_f32" if fast else "_generic"
    names = {TAG_PREFIX + "stats": "k_gat_edge_attn_stats" + sfx(ok and not case.shuffled)}   # needs a row_owned plan
    for tag in ("fwd", "bwd_row", "bwd_col"):
        names[TAG_PREFIX + drop + tag] = "k_gat_edge_attn_" + drop + tag + sfx(ok)
    names[TAG_PREFIX + "pack"] = "k_gat_attn_pack" + sfx(ok)
    return names


def all_fast(case):
    return all(k.endswith("_f32") for k in expected_kernels(case).values())


def bounds(case):
    """dict(rtol, atol): gat_edge_reference.TOL32 with atol / (1 - p) as gat_fuzz.bounds, or TOL64"""
    if case.dtype == "float64":
        return dict(E.TOL64)
    return dict(rtol=E.TOL32["rtol"], atol=E.TOL32["atol"] / (1 - case.p))


# ---- graph and inputs ----------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class EdgeBuilt(Built):
    src: torch.Tensor       # the edge list in EDGE-ID order (what gat_edge_reference takes): edge e joins row src[e] and
    dst: torch.Tensor       # neighbour dst[e] and owns ee[e]


def number_edges(case, g):
    """(g', src, dst) by the case's numbering"""
    if case.numbering == "row_identity":
        return E.permute_edge_ids(g, None)
    if case.numbering == "col_identity":
        return E.column_identity_edge_ids(g)
    assert case.numbering == "permuted"
    return E.permute_edge_ids(g, case.input_seed + 2)


def build(case, n_cu):
    """The case's graph (large stratum: sized for n_cu compute units), numbered, and its inputs."""
    g, src, dst = number_edges(case, F.drawn_graph(case, n_cu))
    csr = F.chunk_lists(case, g)
    dt = case.torch_dtype
    *tables, grad = E.inputs(src, dst, g.n_src, g.n_dst, case.h, case.d, dt, case.input_seed, case.kind)
    if case.large:
        grad = grad * F.LARGE_GRAD_SCALE
    if case.kind == "ties":
        grad = grad * TIES_GRAD_SCALE
    return EdgeBuilt(g, csr, tuple(tables), F._view_values(grad, case.grad_view), src, dst)


# ---- the reference, one head at a time -------------------------------------------------------------------------------
def reference(case, built, dtype=torch.float64):
    """{output name: expected tensor} by autograd through gat_edge_reference.gat_edge_layer in `dtype`"""
    src, dst, g = built.src, built.dst, built.g
    sel, join, _ = F._per_head(built.inputs[0], 1)
    mult = DR.multipliers(src.numpy(), dst.numpy(), len(sel), case.p, case.philox_seed, case.offset,
                          dtype) if case.dropped else None
    outs = [[] for _ in range(5)]
    for k, head in enumerate(sel):
        r = [head(t).to(dtype).clone().requires_grad_(True) for t in built.inputs]
        o = E.gat_edge_layer(src, dst, g.n_src, r[0], r[1], r[2], r[3], case.slope,
                             None if mult is None else mult[:, k:k + 1])
        o.backward(head(built.grad).to(dtype))
        for lst, t in zip(outs, (o.detach(), r[0].grad, r[1].grad, r[2].grad, r[3].grad)):
            lst.append(t)
    return dict(zip(OUTPUTS, (join(ts) for ts in outs)))


def ratios(case, got, want):
    """{output name: used fraction of its bound}; dee only where the case asks for it"""
    tol = bounds(case)
    return {name: F.R.ratio(got[name], want[name], tol) for name in OUTPUTS
            if name in got and (name != "dee" or case.need_dee)}


@functools.lru_cache(maxsize=None)
def case_data(seed, n_cu):
    """(case, built, float64 reference) of a seed, computed once per process and left unchanged"""
    case = draw(seed)
    built = build(case, n_cu)
    return case, built, reference(case, built)


# ---- the call on the device ----------------------------------------------------------------------------------------------
set_knobs = F.set_knobs
assert_cpg = F.assert_cpg


def run(case, built, dev):
    """One forward and backward of the case on `dev` through its drawn entry -> {output name: tensor}; with
    need_dee = False the raw ops get need_dee=False (dee is an empty (0,) tensor) and the autograd entry leaves
    ee.requires_grad false (dee is None)."""
    from custom_op_benchmark_amd import functions, graphop as ops
    a8 = tuple(t.to(dev) for t in built.csr)
    x = [t.to(dev) for t in built.inputs]
    if case.misaligned >= 0:
        x[case.misaligned] = off_boundary(x[case.misaligned])
    grad = built.grad.to(dev)
    drop = (case.p, case.philox_seed, case.offset)
    if case.entry == "autograd":
        el, er, ee, V = x
        for t in (el, er, V):
            t.requires_grad_(True)
        ee.requires_grad_(case.need_dee)
        o = functions.fused_gat_edge_attention_step(_Csr(a8), el, er, ee, V, as_view(grad, case.grad_view), case.slope,
                                                    *drop)
        assert (ee.grad is not None) == case.need_dee
        return dict(zip(OUTPUTS, (o.detach(), el.grad, er.grad, ee.grad, V.grad)))
    m = {"ctypes": ops, "cpp_ext": ops.cpp_ext if ops.cpp_ext is not None else ops, "torch_ops": torch.ops.graphop}[
        case.entry]
    o, stats = m.gat_edge_attention_forward(*a8[:4], *x, case.slope, *drop)
    grads = list(m.gat_edge_attention_backward(*a8, *x, o, stats, grad, case.slope, *drop, case.need_dee))
    if not case.need_dee:
        assert grads[2].shape == (0,) and grads[2].dtype == case.torch_dtype
    out = dict(zip(OUTPUTS, [o] + grads))
    out["stats"] = stats
    return out
