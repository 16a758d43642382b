"""autograd glue: the reference's four ``torch.autograd.Function`` classes.

Same class names, ``.apply`` argument orders and gradient routing as ``wrapper.py:8-55``: index
tensors get ``None`` gradients; ``MaskedMMCSR`` returns ``(dA, dB)`` last, ``VectorSPMM``
``(dedata, dx)`` last, ``SparseSoftmax`` a 4-tuple, ``NodeMulEdge`` a 5-tuple.  They call this
package's HIP ops instead of the CUDA extension.
"""
import torch
from torch.autograd import Function

from . import _lib
from . import graphop as _ops


class SparseSoftmax(Function):
    """y = softmax of edge values per row; apply(row, indptr, eid, x)   (wrapper.py:8-18)"""

    @staticmethod
    def forward(ctx, row, indptr, eid, x):
        y = _ops.sparse_softmax_forward(row, indptr, eid, x)
        ctx.save_for_backward(row, indptr, eid, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        row, indptr, eid, y = ctx.saved_tensors
        return None, None, None, _ops.sparse_softmax_backward(row, indptr, eid, y, dy)


class MaskedMMCSR(Function):
    """SDDMM; apply(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, A, B)
    (wrapper.py:20-30)"""

    @staticmethod
    def forward(ctx, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, A, B):
        ctx.save_for_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, A, B)
        return _ops.maskedmm_csr_forward(row, indptr_r, eid_r, indices_r, A, B)

    @staticmethod
    def backward(ctx, grad):
        row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, A, B = ctx.saved_tensors
        dA, dB = _ops.maskedmm_csr_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c,
                                            indices_c, A, B, grad)
        return None, None, None, None, None, None, None, None, dA, dB


class NodeMulEdge(Function):
    """apply(row, indptr, eid, A, B)   (wrapper.py:32-42)"""

    @staticmethod
    def forward(ctx, row, indptr, eid, A, B):
        ctx.save_for_backward(row, indptr, eid, A, B)
        return _ops.node_mul_edge_forward(row, indptr, eid, A, B)

    @staticmethod
    def backward(ctx, grad):
        row, indptr, eid, A, B = ctx.saved_tensors
        dA, dB = _ops.node_mul_edge_backward(row, indptr, eid, A, B, grad)
        return None, None, None, dA, dB


class VectorSPMM(Function):
    """apply(row, indptr, eid, indices, col, ptr_t, eid_t, indices_t, edata, x)
    (wrapper.py:44-55)"""

    @staticmethod
    def forward(ctx, row, indptr, eid, indices, col, ptr_t, eid_t, indices_t, edata, x):
        y = _ops.vector_spmm_forward(row, indptr, eid, indices, edata, x)
        ctx.save_for_backward(row, indptr, eid, indices, col, ptr_t, eid_t, indices_t, edata, x)
        return y

    @staticmethod
    def backward(ctx, dy):
        row, indptr, eid, indices, col, ptr_t, eid_t, indices_t, edata, x = ctx.saved_tensors
        dedata, dx = _ops.vector_spmm_backward(row, indptr, eid, indices, col, ptr_t, eid_t,
                                               indices_t, edata, dy.contiguous(), x)
        return None, None, None, None, None, None, None, None, dedata, dx


class GATScores(Function):
    """GAT additive attention scores s = LeakyReLU(el[i] + er[j]) per edge and head (extra op, not in the reference):
    apply(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, negative_slope).  el (n_src[, h]),
    er (n_dst[, h]); s is (E) for one head, else (E, h) -- the edge layout SparseSoftmax and VectorSPMM take.  Saves the
    CSR arrays, el and er only: the backward recomputes the pre-activation per slot."""

    @staticmethod
    def forward(ctx, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, negative_slope):
        ctx.save_for_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er)
        ctx.negative_slope = float(negative_slope)
        return _ops.gat_scores_forward(row, indptr_r, eid_r, indices_r, el, er, ctx.negative_slope)

    @staticmethod
    def backward(ctx, grad):
        a8, (el, er) = ctx.saved_tensors[:8], ctx.saved_tensors[8:]
        d_el, d_er = _ops.gat_scores_backward(*a8, el, er, grad, ctx.negative_slope)
        return None, None, None, None, None, None, None, None, d_el, d_er, None


class GATv2Scores(Function):
    """GATv2 attention scores s = sum_c att[k, c] * LeakyReLU(xl[i, k, c] + xr[j, k, c]) per edge and head (extra op, not in
    the reference): apply(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, att, negative_slope).
    xl (n_src, d), xr (n_dst, d), att (d) for one head, else (n, h, d) and (h, d); s is (E) for one head, else (E, h) --
    the edge layout SparseSoftmax and VectorSPMM take.  Saves the CSR arrays, xl, xr and att only: the backward
    recomputes the pre-activation per slot."""

    @staticmethod
    def forward(ctx, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, att, negative_slope):
        ctx.save_for_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, att)
        ctx.negative_slope = float(negative_slope)
        return _ops.gatv2_scores_forward(row, indptr_r, eid_r, indices_r, xl, xr, att, ctx.negative_slope)

    @staticmethod
    def backward(ctx, grad):
        a8, (xl, xr, att) = ctx.saved_tensors[:8], ctx.saved_tensors[8:]
        dxl, dxr, datt = _ops.gatv2_scores_backward(*a8, xl, xr, att, grad, ctx.negative_slope)
        return None, None, None, None, None, None, None, None, dxl, dxr, datt, None


class FusedGATAttention(Function):
    """o = VectorSPMM(SparseSoftmax(GATScores(el, er)), V) as ONE autograd node (extra op, not in the reference):
    apply(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, V, negative_slope).  el (n_src[, h]),
    er (n_dst[, h]), V (n_dst, d) for one head, else (n_dst, h, d); o has n_src rows in V's layout.  Saves (el, er, V, o,
    row statistics) instead of any (E, h) tensor; the backward recomputes the attention weights per slot."""

    @staticmethod
    def forward(ctx, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, V, negative_slope):
        o, stats = _ops.gat_attention_forward(row, indptr_r, eid_r, indices_r, el, er, V, float(negative_slope))
        ctx.save_for_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, V, o, stats)
        ctx.negative_slope = float(negative_slope)
        return o

    @staticmethod
    def backward(ctx, dO):
        a8, (el, er, V, o, stats) = ctx.saved_tensors[:8], ctx.saved_tensors[8:]
        d_el, d_er, dV = _ops.gat_attention_backward(*a8, el, er, V, o, stats, dO, ctx.negative_slope)
        return None, None, None, None, None, None, None, None, d_el, d_er, dV, None


class FusedGATv2Attention(Function):
    """o = VectorSPMM(SparseSoftmax(GATv2Scores(xl, xr, att)), xr) as ONE autograd node (extra op, not in the reference):
    apply(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, att, negative_slope).  xl (n_src, d),
    xr (n_dst, d), att (d) for one head, else (n, h, d) and (h, d); o has n_src rows in xl's layout.  The aggregated table
    is xr itself (the GATv2Conv convention; gatv2_attention_step serves a separate V).  Saves the CSR arrays, xl, xr,
    att, o and the row statistics instead of any (E, h) tensor; the backward recomputes scores and weights per slot."""

    @staticmethod
    def forward(ctx, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, att, negative_slope):
        o, stats = _ops.gatv2_attention_forward(row, indptr_r, eid_r, indices_r, xl, xr, att, float(negative_slope))
        ctx.save_for_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, att, o, stats)
        ctx.negative_slope = float(negative_slope)
        return o

    @staticmethod
    def backward(ctx, dO):
        a8, (xl, xr, att, o, stats) = ctx.saved_tensors[:8], ctx.saved_tensors[8:]
        dxl, dxr, datt = _ops.gatv2_attention_backward(*a8, xl, xr, att, o, stats, dO, ctx.negative_slope)
        return None, None, None, None, None, None, None, None, dxl, dxr, datt, None


class FusedGATAttentionDropout(Function):
    """FusedGATAttention with dropout on the attention weights, o[i] = sum_j a_ij m_ij V[j] (extra op):
    apply(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, V, negative_slope, p, seed, offset).
    m_ij = keep / (1 - p), the keep decision a pure function of (i, j, head, seed, offset, p) that forward and backward
    recompute per slot (Philox4x32-10; graphop.edge_dropout_mask gives the same values as an edge tensor), so still no
    (E, h) tensor is kept or made.  seed=None draws one from torch's default CPU generator (torch.manual_seed makes
    runs repeatable); offset is a per-layer / per-step counter, so one seed serves a whole model."""

    @staticmethod
    def forward(ctx, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, V, negative_slope, p,
                seed=None, offset=0):
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        ctx.drop = (float(negative_slope), float(p), int(seed), int(offset))
        o, stats = _ops.gat_attention_dropout_forward(row, indptr_r, eid_r, indices_r, el, er, V, *ctx.drop)
        ctx.save_for_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, V, o, stats)
        return o

    @staticmethod
    def backward(ctx, dO):
        a8, (el, er, V, o, stats) = ctx.saved_tensors[:8], ctx.saved_tensors[8:]
        d_el, d_er, dV = _ops.gat_attention_dropout_backward(*a8, el, er, V, o, stats, dO, *ctx.drop)
        return None, None, None, None, None, None, None, None, d_el, d_er, dV, None, None, None, None


class FusedGATv2AttentionDropout(Function):
    """FusedGATv2Attention with dropout on the attention weights, o[i] = sum_j a_ij m_ij xr[j] (extra op):
    apply(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, att, negative_slope, p, seed, offset).
    m_ij is the multiplier of FusedGATAttentionDropout (i indexes xl, j indexes xr; graphop.edge_dropout_mask gives the
    same values as an edge tensor), recomputed per slot by forward and backward, so still no (E, h) tensor is kept or
    made; saves exactly what FusedGATv2Attention saves.  seed=None draws one from torch's default CPU generator
    (torch.manual_seed makes runs repeatable); offset is a per-layer / per-step counter."""

    @staticmethod
    def forward(ctx, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, att, negative_slope, p,
                seed=None, offset=0):
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        ctx.drop = (float(negative_slope), float(p), int(seed), int(offset))
        o, stats = _ops.gatv2_attention_dropout_forward(row, indptr_r, eid_r, indices_r, xl, xr, att, *ctx.drop)
        ctx.save_for_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, att, o, stats)
        return o

    @staticmethod
    def backward(ctx, dO):
        a8, (xl, xr, att, o, stats) = ctx.saved_tensors[:8], ctx.saved_tensors[8:]
        dxl, dxr, datt = _ops.gatv2_attention_dropout_backward(*a8, xl, xr, att, o, stats, dO, *ctx.drop)
        return None, None, None, None, None, None, None, None, dxl, dxr, datt, None, None, None, None


class FusedGATEdgeAttention(Function):
    """The fused GAT layer with a per-edge score term (extra op; GATConv(edge_dim=...) / EGATConv, or a fixed per-edge
    bias such as log edge weights):
    apply(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, ee, V, negative_slope, p, seed, offset)
    -> o[i] = sum_j softmax_j(LeakyReLU(el[i] + er[j] + ee[e])) m_ij V[j] for edge e = (i, j), ee indexed by edge id.
    m_ij is the multiplier of FusedGATAttentionDropout (1 at p = 0; seed=None draws one from torch's default CPU
    generator).  Saves the CSR arrays, el, er, ee, V, o and stats only; the backward makes one edge-sized tensor, the
    gradient of ee, and none when ee does not require grad."""

    @staticmethod
    def forward(ctx, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, ee, V, negative_slope,
                p=0.0, seed=None, offset=0):
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        ctx.drop = (float(negative_slope), float(p), int(seed), int(offset))
        o, stats = _ops.gat_edge_attention_forward(row, indptr_r, eid_r, indices_r, el, er, ee, V, *ctx.drop)
        ctx.save_for_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, ee, V, o, stats)
        return o

    @staticmethod
    def backward(ctx, dO):
        a8, (el, er, ee, V, o, stats) = ctx.saved_tensors[:8], ctx.saved_tensors[8:]
        need_dee = ctx.needs_input_grad[10]
        d_el, d_er, d_ee, dV = _ops.gat_edge_attention_backward(*a8, el, er, ee, V, o, stats, dO, *ctx.drop,
                                                                need_dee=need_dee)
        return (None,) * 8 + (d_el, d_er, d_ee if need_dee else None, dV, None, None, None, None)


class FusedGATv2EdgeAttention(Function):
    """The fused GATv2 layer with edge features (extra op; GATv2Conv(edge_dim=...)):
    apply(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, xe, att, negative_slope, p, seed, offset)
    -> o[i] = sum_j softmax_j(att . LeakyReLU(xl[i] + xr[j] + xe[e])) m_ij xr[j] for edge e = (i, j), xe indexed by edge
    id: (n_edges, d) for 2-D xl / xr, else (n_edges, h, d).  m_ij is the multiplier of FusedGATAttentionDropout (1 at
    p = 0; seed=None draws one from torch's default CPU generator).  Saves the CSR arrays, xl, xr, xe, att, o and stats
    only; the backward makes one edge-sized tensor, the gradient of xe, and none when xe does not require grad."""

    @staticmethod
    def forward(ctx, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, xe, att, negative_slope,
                p=0.0, seed=None, offset=0):
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        ctx.drop = (float(negative_slope), float(p), int(seed), int(offset))
        o, stats = _ops.gatv2_attention_dropout_forward(row, indptr_r, eid_r, indices_r, xl, xr, att, *ctx.drop, xe=xe)
        ctx.save_for_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, xe, att, o, stats)
        return o

    @staticmethod
    def backward(ctx, dO):
        a8, (xl, xr, xe, att, o, stats) = ctx.saved_tensors[:8], ctx.saved_tensors[8:]
        need_dxe = ctx.needs_input_grad[10]
        dxl, dxr, datt, dxe = _ops.gatv2_attention_dropout_backward(*a8, xl, xr, att, o, stats, dO, *ctx.drop, xe=xe,
                                                                    need_dxe=need_dxe)
        return (None,) * 8 + (dxl, dxr, dxe if need_dxe else None, datt, None, None, None, None)


# FusedAttention over several heads (round 5): "keep" = per head group only a_g (E x hg) survives the forward, the backward's
# da_g / ds_g are E x hg temporaries -- speed of the 8-function step, about half of its E-sized memory; "recompute" = nothing
# E-sized survives the forward, the backward recomputes s_g and a_g per group (two more passes per group: ~+17 % time,
# about a third of the 8-function step's E-sized memory).  Set before the forward; GRAPHOP_FUSED_HEADS overrides.
FUSED_HEADS_MODE = "keep"


def _head_group(h, d, n_edges=None, n_nodes=None):
    """Heads per group of the head-blocked FusedAttention: rows of hg x d floats = 256 B where d allows (the row width
    every driver is fastest at per byte: Reddit-shape 2 x 32 runs 13.6 ms against 55.4 / 4 at 8 x 32), one head per
    group from d = 64 on (d = 64: the one-head fused kernels then apply to every head).  hg divides h; hg == h: no blocking.
    With the graph's size given, blocking is only chosen where it SAVES memory: it trades (E, h)-sized temporaries
    (2 E (h - hg) floats) for about seven node-sized copies per group (7 n hg d floats) -- on graphs of few edges per
    node the node tensors are the big ones (products-shape 8 x 16, E / n = 25: measured 1.5 x the 8-function step's peak
    and +18 % time with groups of 4, tools/fused_heads_memory.py), so the margin is a factor two."""
    want = max(1, 64 // max(1, d))
    hg = 1
    for c in range(1, h + 1):
        if h % c == 0 and c <= want:
            hg = c
    if n_edges is not None and n_nodes and hg < h and 2 * n_edges * (h - hg) < 2 * 7 * n_nodes * hg * d:
        return h
    return hg


def _heads_per_call(a8, Q, K, h):
    """Heads per call of the three fused attention classes.  Where the whole (n, h, d) call takes the several-head
    kernels (attention_backward_is_fused says so for h > 1) that is h: ONE call, no head slices, db
    written straight into one (E, h) tensor.  Otherwise _head_group's value, as before."""
    if h <= 1:
        return 1
    if _ops.attention_backward_is_fused(*a8, Q, K):
        return h
    return _head_group(h, Q.size(-1), a8[2].numel(), max(Q.size(0), K.size(0)))


class FusedAttention(Function):
    """o = VectorSPMM(SparseSoftmax(MaskedMMCSR(Q, K)), V) as ONE autograd node (extra op, not in the
    reference): apply(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V).
    Saves (Q, K, V, o, row statistics) instead of the E-sized s / a; the backward recomputes them
    inside two fused passes.
    Several heads (the reference's second benchmarked layout is 8 x 64, wrapper.py:306-309; BASELINE config 3 is 8 x 128)
    are processed in HEAD GROUPS (round 5): a group's heads are copied to contiguous (n, hg, d) tensors (node-sized
    copies), run through this op's one-group form -- the fused kernels where they apply (one head of d <= 64), the
    unfused entry points otherwise -- and written back into the heads' slices of o / dQ / dK / dV.  No (E, h) tensor
    ever exists: the E-sized temporaries are (E, hg), one group at a time (FUSED_HEADS_MODE).
    Where the several-head kernels apply (fp32, (h, d) one of their pairs) the whole call is ONE fused
    call instead (_heads_per_call): no head groups, no slices, nothing edge-sized at all."""

    @staticmethod
    def forward(ctx, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V):
        a8 = (row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c)
        h = Q.size(1) if Q.dim() == 3 else 1
        hg = _heads_per_call(a8, Q, K, h)
        ctx.groups = None
        if h > 1 and hg < h:
            return _groups_forward(ctx, a8, Q, K, V, h, hg)
        # (fewer key rows than query rows: the unfused SpMM returns zeros_like(V) and cannot hold o; the raw op can, and
        #  composes inside the library where no fused form applies)
        ctx.fused = _ops.attention_backward_is_fused(*a8, Q, K) or K.size(0) < Q.size(0)
        if ctx.fused:
            o, stats = _ops.attention_forward(row, indptr_r, eid_r, indices_r, Q, K, V)
            ctx.save_for_backward(*a8, Q, K, V, o, stats)
        else:
            # the fused passes do not apply (fp64, short rows, one group of several heads ...): keep a for the unfused
            # backward ops instead of letting attention_backward recompute s and a
            s = _ops.maskedmm_csr_forward(row, indptr_r, eid_r, indices_r, Q, K)
            a = _ops.sparse_softmax_forward(row, indptr_r, eid_r, s)
            del s
            o = _ops.vector_spmm_forward(row, indptr_r, eid_r, indices_r, a, V)
            if o.size(0) != Q.size(0):
                o = o[:Q.size(0)]
            ctx.save_for_backward(*a8, Q, K, V, a)
        return o

    @staticmethod
    def backward(ctx, dO):
        a8, rest = ctx.saved_tensors[:8], ctx.saved_tensors[8:]
        row, indptr_r, eid_r = a8[:3]
        if ctx.groups is not None:
            return (None,) * 8 + _groups_backward(ctx, a8, *rest, dO)
        if ctx.fused:
            Q, K, V, o, stats = rest
            dQ, dK, dV = _ops.attention_backward(*a8, Q, K, V, o, stats, dO)
        else:
            Q, K, V, a = rest
            da, dV = _ops.vector_spmm_backward(*a8, a, dO.contiguous(), V)
            ds = _ops.sparse_softmax_backward(row, indptr_r, eid_r, a, da)
            del da
            dQ, dK = _ops.maskedmm_csr_backward(*a8, Q, K, ds)
        return None, None, None, None, None, None, None, None, dQ, dK, dV


def _drop_seed(seed, p):
    """the seed of a fused attention class: the caller's, or with seed=None one drawn from torch's default CPU generator
    (only where p > 0 uses it; else 0)"""
    if seed is not None:
        return seed
    return int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item()) if float(p) > 0.0 else 0


class FusedAttentionDropout(Function):
    """FusedAttention with dropout on the attention weights, o[i] = sum_j softmax_j(<Q_i, K_j>) m_ij V[j] (extra op;
    TransformerConv(dropout=...), DotGatConv):
    apply(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, p, seed, offset).
    m_ij = keep / (1 - p) is the multiplier of FusedGATAttentionDropout (i indexes Q, j indexes K / V; head k of a
    several-head call is head k of graphop.edge_dropout_mask), recomputed per slot by forward and backward: no (E, h)
    mask, and nothing else edge-sized, is kept between them.  Saves (Q, K, V, o, row statistics).  There is no
    1 / sqrt(d) scale argument: fold it into Q.  seed=None draws one from torch's default CPU generator; offset is a
    per-layer / per-step counter.  p = 0 is FusedAttention itself.
    Several heads take the several-head kernels in one call where they apply (_heads_per_call), else they run in
    FusedAttention's head groups (_head_group) and each group's call names its first head, so a grouped call makes the
    decisions of an ungrouped one.  FUSED_HEADS_MODE is honoured as far as it can be: a group the
    fused kernels do not take recomputes s and a in the backward in both modes (keeping a would not spare the mask)."""

    @staticmethod
    def forward(ctx, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, p, seed=None, offset=0):
        a8 = (row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c)
        ctx.drop = None
        if float(p) == 0.0:
            return FusedAttention.forward(ctx, *a8, Q, K, V)
        seed = _drop_seed(seed, p)
        ctx.drop = (float(p), int(seed), int(offset))
        h = Q.size(1) if Q.dim() == 3 else 1
        hg = _heads_per_call(a8, Q, K, h)
        ctx.groups = None
        if h > 1 and hg < h:
            return _groups_forward(ctx, a8, Q, K, V, h, hg, ctx.drop)
        o, stats = _ops.attention_dropout_forward(row, indptr_r, eid_r, indices_r, Q, K, V, *ctx.drop, 0)
        ctx.save_for_backward(*a8, Q, K, V, o, stats)
        return o

    @staticmethod
    def backward(ctx, dO):
        if ctx.drop is None:
            return FusedAttention.backward(ctx, dO) + (None, None, None)
        a8, rest = ctx.saved_tensors[:8], ctx.saved_tensors[8:]
        if ctx.groups is not None:
            return (None,) * 8 + _groups_backward(ctx, a8, *rest, dO, ctx.drop) + (None, None, None)
        Q, K, V, o, stats = rest
        dQ, dK, dV = _ops.attention_dropout_backward(*a8, Q, K, V, o, stats, dO, *ctx.drop, 0)
        return (None,) * 8 + (dQ, dK, dV, None, None, None)


class FusedAttentionBias(Function):
    """FusedAttentionDropout with a term per edge inside the softmax (extra op): for edge e = (i, j)
    and head k,  s_e = <Q_i, K_j> + b[e, k],  o[i] = sum_e softmax_e(s) m_e V[j]:
    apply(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, b, p=0.0, seed=None, offset=0).
    b is indexed by edge id -- (E) with 2-D Q / K / V, (E, h) with 3-D ones -- in their dtype.  Uses: a Graphormer-type
    bias (spatial and edge encodings), a relative positional bias, a weighted graph with b = log w, and the key-side
    edge term of TransformerConv(edge_dim=...), b = node_mul_edge_forward(Q, xe) (through NodeMulEdge, so that its
    backward turns db into the gradients of Q and xe) -- the key side ALONE: that layer also adds the edge row to the
    value, which no bias can express; FusedAttentionEdge has both terms.  For a CATEGORICAL bias (b = B[etype]: distance
    buckets, bond types, relations) use FusedAttentionTypeBias, which takes the table and the types and makes neither b
    nor db.  b must be finite: a bias at or below the -1e9 floor of the row
    maximum is not a mask.  Saves (Q, K, V, b, o, row statistics) and nothing edge-sized but b; the backward makes db
    = ds only where b needs a gradient.  m_e is FusedAttentionDropout's multiplier (1 at p = 0: no dropout); seed=None
    draws one from torch's default CPU generator.  There is no 1 / sqrt(d) scale argument: fold it into Q.
    Several heads take the several-head kernels in one call where they apply (_heads_per_call: no slices, db written
    once into one (E, h) tensor); else they run in FusedAttention's head groups (_head_group): a group gets the
    contiguous slice b[:, g0:g0 + hg] (an (E, hg) copy), writes its db into its slice of one (E, h) result and names
    its first head."""

    @staticmethod
    def forward(ctx, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, b, p=0.0, seed=None,
                offset=0):
        a8 = (row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c)
        seed = _drop_seed(seed, p)
        ctx.drop = (float(p), int(seed), int(offset))
        h = Q.size(1) if Q.dim() == 3 else 1
        hg = _heads_per_call(a8, Q, K, h)
        ctx.groups = None
        if h > 1 and hg < h:
            return _groups_forward(ctx, a8, Q, K, V, h, hg, ctx.drop, b)
        o, stats = _ops.attention_bias_forward(row, indptr_r, eid_r, indices_r, Q, K, V, b, *ctx.drop, 0)
        ctx.save_for_backward(*a8, Q, K, V, b, o, stats)
        return o

    @staticmethod
    def backward(ctx, dO):
        a8, rest = ctx.saved_tensors[:8], ctx.saved_tensors[8:]
        need_db = ctx.needs_input_grad[11]
        if ctx.groups is not None:
            Q, K, V, b = rest
            dQ, dK, dV, db = _groups_backward(ctx, a8, Q, K, V, dO, ctx.drop, b, need_db)
        else:
            Q, K, V, b, o, stats = rest
            dQ, dK, dV, db = _ops.attention_bias_backward(*a8, Q, K, V, b, o, stats, dO, *ctx.drop, 0, need_db)
        return (None,) * 8 + (dQ, dK, dV, db if need_db else None, None, None, None)


class FusedAttentionEdge(Function):
    """FusedAttentionDropout with a feature row per edge added to the key AND the value (extra op): for
    edge e = (i, j) and head k,  kx = K[j] + xe[e],  vx = V[j] + xe[e],  s_e = <Q_i, kx_e>,  o[i] = sum_e softmax_e(s) m_e vx_e:
    apply(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, xe, p=0.0, seed=None, offset=0).
    xe is indexed by edge id -- (E, d) with 2-D Q / K / V, (E, h, d) with 3-D ones -- in their dtype, contiguous: the
    projected edge_attr of TransformerConv(edge_dim=...), of the Dwivedi-Bresson graph transformer, of GraphGPS.  Saves
    the CSR arrays, (Q, K, V, xe, o, row statistics) and nothing else; the backward makes dxe = ds Q_i + a m dO_i, the only
    edge-sized tensor, and only where xe needs a gradient.  m_e is FusedAttentionDropout's multiplier (1 at p = 0: no
    dropout); seed=None draws one from torch's default CPU generator.  There is no 1 / sqrt(d) scale argument: fold it
    into Q.  One call whatever h: there are no head groups.  For a CATEGORICAL edge feature (xe = R[etype]: relations,
    bond types, clipped relative positions) use FusedAttentionEdgeType, which takes the table and the types and makes
    neither xe nor dxe."""

    @staticmethod
    def forward(ctx, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, xe, p=0.0, seed=None,
                offset=0):
        a8 = (row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c)
        seed = _drop_seed(seed, p)
        ctx.drop = (float(p), int(seed), int(offset))
        o, stats = _ops.attention_edge_forward(row, indptr_r, eid_r, indices_r, Q, K, V, xe, *ctx.drop, 0)
        ctx.save_for_backward(*a8, Q, K, V, xe, o, stats)
        return o

    @staticmethod
    def backward(ctx, dO):
        a8, (Q, K, V, xe, o, stats) = ctx.saved_tensors[:8], ctx.saved_tensors[8:]
        need_dxe = ctx.needs_input_grad[11]
        dQ, dK, dV, dxe = _ops.attention_edge_backward(*a8, Q, K, V, xe, o, stats, dO, *ctx.drop, 0, need_dxe)
        return (None,) * 8 + (dQ, dK, dV, dxe if need_dxe else None, None, None, None)


class FusedAttentionEdgeType(Function):
    """FusedAttentionEdge for a categorical edge feature (extra op): edge e = (i, j) carries the type
    t = etype[e] and the row R[t] of a learned table is added to its key AND its value,  kx = K[j] + R[t],
    vx = V[j] + R[t],  s_e = <Q_i, kx_e>,  o[i] = sum_e softmax_e(s) m_e vx_e:
    apply(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, R, etype, p=0.0, seed=None, offset=0).
    etype is (E) torch.int32 by edge id with values in [0, n_types); R is (n_types, d) with 2-D Q / K / V, (n_types, h, d)
    with 3-D ones, in their dtype, contiguous: an nn.Embedding's weight (relation-aware attention, Shaw-type relative
    positions, TransformerConv(edge_dim=...) behind an embedding).  It is FusedAttentionEdge on R[etype.long()] without
    that (E, h, d) tensor and without its gradient: R.grad[t] = sum over the edges of type t of (ds Q_i + a m dO_i) is
    summed on chip, and only where R needs a gradient.  Saves the CSR arrays, (Q, K, V, R, etype, o, row statistics) and
    nothing else; etype gets no gradient.  Types outside [0, n_types) are not detected (that would synchronise): the
    kernels clamp them, so they give undefined values and touch no memory outside R / R.grad.  m_e, seed=None and the
    missing 1 / sqrt(d) argument: as FusedAttentionEdge.  One call whatever h."""

    @staticmethod
    def forward(ctx, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, R, etype, p=0.0,
                seed=None, offset=0):
        a8 = (row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c)
        seed = _drop_seed(seed, p)
        ctx.drop = (float(p), int(seed), int(offset))
        o, stats = _ops.attention_etype_forward(row, indptr_r, eid_r, indices_r, Q, K, V, R, etype, *ctx.drop, 0)
        ctx.save_for_backward(*a8, Q, K, V, R, etype, o, stats)
        return o

    @staticmethod
    def backward(ctx, dO):
        a8, (Q, K, V, R, etype, o, stats) = ctx.saved_tensors[:8], ctx.saved_tensors[8:]
        need_dR = ctx.needs_input_grad[11]
        dQ, dK, dV, dR = _ops.attention_etype_backward(*a8, Q, K, V, R, etype, o, stats, dO, *ctx.drop, 0, need_dR)
        return (None,) * 8 + (dQ, dK, dV, dR if need_dR else None, None, None, None, None)


class FusedAttentionTypeBias(Function):
    """FusedAttentionBias for a categorical edge feature whose learned term is one scalar per (category, head) (extra
    op): edge e = (i, j) carries the type t = etype[e] and, for head k,  s_e = <Q_i, K_j> + B[t, k],
    o[i] = sum_e softmax_e(s) m_e V[j]:
    apply(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, B, etype, p=0.0, seed=None, offset=0).
    etype is (E) torch.int32 by edge id with values in [0, n_types); B is (n_types) with 2-D Q / K / V, (n_types, h) with
    3-D ones, in their dtype, contiguous and finite: an nn.Embedding's weight (Graphormer's spatial encoding and its edge
    encoding on bond types, T5 / Swin-type bucketed relative positions, relation biases).  It is FusedAttentionBias on
    B[etype.long()] without that (E, h) tensor and without its gradient: B.grad[t] = sum over the edges of type t of ds
    is summed on chip, and only where B needs a gradient.  One call whatever h: there are no head groups.  Saves the CSR
    arrays, (Q, K, V, B, etype, o, row statistics) and nothing else; etype gets no gradient.  Types outside
    [0, n_types) are not detected (that would synchronise): the kernels clamp them, so they give undefined values and
    touch no memory outside B / B.grad.  m_e, seed=None and the missing 1 / sqrt(d) argument: as FusedAttentionBias."""

    @staticmethod
    def forward(ctx, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, B, etype, p=0.0,
                seed=None, offset=0):
        a8 = (row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c)
        seed = _drop_seed(seed, p)
        ctx.drop = (float(p), int(seed), int(offset))
        o, stats = _ops.attention_tbias_forward(row, indptr_r, eid_r, indices_r, Q, K, V, B, etype, *ctx.drop, 0)
        ctx.save_for_backward(*a8, Q, K, V, B, etype, o, stats)
        return o

    @staticmethod
    def backward(ctx, dO):
        a8, (Q, K, V, B, etype, o, stats) = ctx.saved_tensors[:8], ctx.saved_tensors[8:]
        need_dB = ctx.needs_input_grad[11]
        dQ, dK, dV, dB = _ops.attention_tbias_backward(*a8, Q, K, V, B, etype, o, stats, dO, *ctx.drop, 0, need_dB)
        return (None,) * 8 + (dQ, dK, dV, dB if need_dB else None, None, None, None, None)


class FusedAttentionWeights(Function):
    """The fused dot-product attention layer that also returns its attention weights (extra op; PyG's
    return_attention_weights=True, DGL's get_attention=True):
    apply(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, b=None, xe=None, p=0.0, seed=None,
    offset=0) -> (o, a).  The mode follows the optional operand: neither is FusedAttentionDropout, b is
    FusedAttentionBias, xe is FusedAttentionEdge (b and xe together are refused); o is that class's o.  a holds the
    UNDROPPED weights by edge id -- (E) with 2-D Q / K / V, else (E, h), SparseSoftmax's layout -- computed from the row
    statistics the forward left (graphop.attention_weights): one SDDMM and one stream pass, or one gather pass with xe,
    not a second softmax.  The effective weights are a * graphop.edge_dropout_mask(...).
    One call of the raw forward whatever h: there are no head groups (a is (E, h) anyway, so they would save nothing).
    Saves the CSR arrays, (Q, K, V, [b | xe], o, row statistics) and NOT a.  The backward takes (dO, ga), either of which
    may be None.  dO goes through the mode's fused backward; without it no fused pass is launched.  In the plain and
    bias modes ga goes through a recomputed a: ds' = a (ga - sum_row a ga) (sparse_softmax_backward; exact, because
    a = softmax(s) whatever produced (m, l)), dQ', dK' = maskedmm_csr_backward(ds'), db' = ds'; the edge-sized
    temporaries a, ga and ds' are inherent once a is an output.  Without ga nothing beyond the fused backward runs.
    With xe, a is marked non-differentiable: its gradient would need sum_e ds'_e xe[e] into dQ and ds'_e Q_i into dxe,
    which nothing in the library does without (E, h, d) temporaries.  seed=None draws one from torch's default CPU
    generator; there is no 1 / sqrt(d) scale argument: fold it into Q."""

    @staticmethod
    def forward(ctx, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, b=None, xe=None, p=0.0,
                seed=None, offset=0):
        a8 = (row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c)
        if b is not None and xe is not None:
            raise RuntimeError("FusedAttentionWeights: at most one of b and xe may be given")
        seed = _drop_seed(seed, p)
        ctx.drop = (float(p), int(seed), int(offset))
        ctx.set_materialize_grads(False)
        ctx.mode = "edge" if xe is not None else ("bias" if b is not None else "plain")
        csr = a8[:4]
        if xe is not None:
            o, stats = _ops.attention_edge_forward(*csr, Q, K, V, xe, *ctx.drop, 0)
        elif b is not None:
            o, stats = _ops.attention_bias_forward(*csr, Q, K, V, b, *ctx.drop, 0)
        else:
            o, stats = _ops.attention_dropout_forward(*csr, Q, K, V, *ctx.drop, 0)
        a = _ops.attention_weights(*csr, Q, K, stats, b, xe)
        extra = () if ctx.mode == "plain" else ((xe,) if xe is not None else (b,))
        ctx.save_for_backward(*a8, Q, K, V, *extra, o, stats)
        if xe is not None:
            ctx.mark_non_differentiable(a)
        return o, a

    @staticmethod
    def backward(ctx, dO, ga):
        a8, rest = ctx.saved_tensors[:8], ctx.saved_tensors[8:]
        row, indptr_r, eid_r, indices_r = a8[:4]
        need_db, need_dxe = ctx.needs_input_grad[11], ctx.needs_input_grad[12]
        db = dxe = None
        if ctx.mode == "edge":
            Q, K, V, xe, o, stats = rest
            if dO is not None:
                dQ, dK, dV, dxe = _ops.attention_edge_backward(*a8, Q, K, V, xe, o, stats, dO, *ctx.drop, 0, need_dxe)
            else:
                dQ, dK, dV = torch.zeros_like(Q), torch.zeros_like(K), torch.zeros_like(V)
                dxe = torch.zeros_like(xe)
            return (None,) * 8 + (dQ, dK, dV, None, dxe if need_dxe else None, None, None, None)
        if ctx.mode == "bias":
            Q, K, V, b, o, stats = rest
        else:
            (Q, K, V, o, stats), b = rest, None
        if dO is None:
            dQ, dK, dV = torch.zeros_like(Q), torch.zeros_like(K), torch.zeros_like(V)
        elif b is not None:
            dQ, dK, dV, db = _ops.attention_bias_backward(*a8, Q, K, V, b, o, stats, dO, *ctx.drop, 0, need_db)
        else:
            dQ, dK, dV = _ops.attention_dropout_backward(*a8, Q, K, V, o, stats, dO, *ctx.drop, 0)
        if ga is not None:
            a = _ops.attention_weights(row, indptr_r, eid_r, indices_r, Q, K, stats, b)
            ds = _ops.sparse_softmax_backward(row, indptr_r, eid_r, a, ga.reshape(a.shape))
            del a
            dQ2, dK2 = _ops.maskedmm_csr_backward(*a8, Q, K, ds)
            dQ += dQ2
            dK += dK2
            if need_db:
                db = ds.reshape(b.shape) if dO is None else db.add_(ds.reshape(b.shape))
        elif need_db and dO is None:
            db = torch.zeros_like(b)
        return (None,) * 8 + (dQ, dK, dV, db if need_db else None, None, None, None, None)


class FusedGATAttentionWeights(Function):
    """The fused GAT layer that also returns its attention weights (extra op; PyG's
    GATConv(..., return_attention_weights=True), DGL's get_attention=True):
    apply(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, V, ee=None, negative_slope=0.2, p=0.0,
    seed=None, offset=0) -> (o, a).  ee=None is FusedGATAttentionDropout, ee is FusedGATEdgeAttention; o is that class's
    o.  a holds the UNDROPPED weights by edge id -- (E) with 1-D el / er, else (E, h), SparseSoftmax's layout -- computed
    from the row statistics the forward left (graphop.gat_attention_weights): one gather pass, not a second softmax.
    The effective weights are a * graphop.edge_dropout_mask(...).
    Saves what the matching class saves -- the CSR arrays, (el, er, [ee,] V, o, row statistics) -- and NOT a.  The backward
    takes (dO, ga), either of which may be None.  dO goes through the matching fused backward; without it no fused pass
    is launched.  ga goes through a recomputed a: ds' = a (ga - sum_row a ga) (sparse_softmax_backward; exact, because
    a = softmax(s) whatever produced (m, l)), then without ee  d_el', d_er' = gat_scores_backward(ds', slope); with ee
    z = gat_scores_forward(el, er, 1) + ee,  dz = z > 0 ? ds' : ds' * slope,  d_el', d_er' = gat_scores_backward(dz, 1)
    and dee' = dz.  The (E, h) temporaries are inherent once a is an output.  The ga terms are added to the fused
    backward's.  seed=None draws one from torch's default CPU generator."""

    @staticmethod
    def forward(ctx, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, V, ee=None,
                negative_slope=0.2, p=0.0, seed=None, offset=0):
        a8 = (row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c)
        ctx.drop = (float(negative_slope), float(p), int(_drop_seed(seed, p)), int(offset))
        ctx.set_materialize_grads(False)
        ctx.edge = ee is not None
        csr = a8[:4]
        if ctx.edge:
            o, stats = _ops.gat_edge_attention_forward(*csr, el, er, ee, V, *ctx.drop)
        else:
            o, stats = _ops.gat_attention_dropout_forward(*csr, el, er, V, *ctx.drop)
        a = _ops.gat_attention_weights(*csr, el, er, stats, ee, ctx.drop[0])
        ctx.save_for_backward(*a8, el, er, *((ee,) if ctx.edge else ()), V, o, stats)
        return o, a

    @staticmethod
    def backward(ctx, dO, ga):
        a8, rest = ctx.saved_tensors[:8], ctx.saved_tensors[8:]
        csr = a8[:4]
        slope = ctx.drop[0]
        need_dee = ctx.edge and ctx.needs_input_grad[11]
        d_ee = None
        if ctx.edge:
            el, er, ee, V, o, stats = rest
        else:
            (el, er, V, o, stats), ee = rest, None
        if dO is None:          # nothing reaches V: its gradient stays None (set_materialize_grads(False))
            d_el, d_er, dV = torch.zeros_like(el), torch.zeros_like(er), None
        elif ctx.edge:
            d_el, d_er, d_ee, dV = _ops.gat_edge_attention_backward(*a8, el, er, ee, V, o, stats, dO, *ctx.drop,
                                                                    need_dee=need_dee)
        else:
            d_el, d_er, dV = _ops.gat_attention_dropout_backward(*a8, el, er, V, o, stats, dO, *ctx.drop)
        if ga is not None:
            a = _ops.gat_attention_weights(*csr, el, er, stats, ee, slope)
            ds = _ops.sparse_softmax_backward(*csr[:3], a, ga.reshape(a.shape))
            del a
            if ctx.edge:
                z = _ops.gat_scores_forward(*csr, el, er, 1.0) + ee
                dz = torch.where(z > 0, ds, ds * slope)
                del z, ds
                d_el2, d_er2 = _ops.gat_scores_backward(*a8, el, er, dz, 1.0)
                if need_dee:
                    d_ee = dz.reshape(ee.shape) if dO is None else d_ee.add_(dz.reshape(ee.shape))
            else:
                d_el2, d_er2 = _ops.gat_scores_backward(*a8, el, er, ds, slope)
            d_el += d_el2
            d_er += d_er2
        elif need_dee and dO is None:
            d_ee = torch.zeros_like(ee)
        return (None,) * 8 + (d_el, d_er, dV, d_ee if need_dee else None, None, None, None, None)


class FusedGATv2AttentionWeights(Function):
    """The fused GATv2 layer that also returns its attention weights (extra op; PyG's
    GATv2Conv(..., return_attention_weights=True), DGL's get_attention=True):
    apply(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, att, xe=None, negative_slope=0.2,
    p=0.0, seed=None, offset=0) -> (o, a).  xe=None is FusedGATv2AttentionDropout, xe is FusedGATv2EdgeAttention; o is that
    class's o.  a holds the UNDROPPED weights by edge id -- (E) with 2-D xl / xr, else (E, h) -- computed from the row
    statistics the forward left (graphop.gatv2_attention_weights): one gather pass that fetches xr[j] per slot and
    streams xe once, not a second softmax and nothing of size (E, h, d).
    Saves what the matching class saves -- the CSR arrays, (xl, xr, [xe,] att, o, row statistics) -- and NOT a.  The
    backward takes (dO, ga), either of which may be None.  dO goes through the matching fused backward; without it no
    fused pass is launched.  Without xe, ga goes through a recomputed a: ds' = a (ga - sum_row a ga)
    (sparse_softmax_backward), dxl', dxr', datt' = gatv2_scores_backward(ds', slope), added to the fused backward's.
    With xe, a is marked non-differentiable: its gradient would need z = xl[i] + xr[j] + xe[e] per edge, (E, h, d)
    temporaries, which is the memory the fused layer exists to avoid.  seed=None draws one from torch's default CPU
    generator."""

    @staticmethod
    def forward(ctx, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, att, xe=None,
                negative_slope=0.2, p=0.0, seed=None, offset=0):
        a8 = (row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c)
        ctx.drop = (float(negative_slope), float(p), int(_drop_seed(seed, p)), int(offset))
        ctx.set_materialize_grads(False)
        ctx.edge = xe is not None
        csr = a8[:4]
        o, stats = _ops.gatv2_attention_dropout_forward(*csr, xl, xr, att, *ctx.drop, xe=xe)
        a = _ops.gatv2_attention_weights(*csr, xl, xr, att, stats, xe, ctx.drop[0])
        ctx.save_for_backward(*a8, xl, xr, *((xe,) if ctx.edge else ()), att, o, stats)
        if ctx.edge:
            ctx.mark_non_differentiable(a)
        return o, a

    @staticmethod
    def backward(ctx, dO, ga):
        a8, rest = ctx.saved_tensors[:8], ctx.saved_tensors[8:]
        csr = a8[:4]
        need_dxe = ctx.edge and ctx.needs_input_grad[11]
        dxe = None
        if ctx.edge:
            xl, xr, xe, att, o, stats = rest
        else:
            (xl, xr, att, o, stats), xe = rest, None
        if dO is None:          # only ga is left, which does not reach xe: its gradient stays None, no (E, h, d) fill
            dxl, dxr, datt = torch.zeros_like(xl), torch.zeros_like(xr), torch.zeros_like(att)
        else:
            dxl, dxr, datt, *more = _ops.gatv2_attention_dropout_backward(*a8, xl, xr, att, o, stats, dO, *ctx.drop,
                                                                          xe=xe, need_dxe=need_dxe)
            if need_dxe:
                dxe = more[0]
        if ga is not None and not ctx.edge:
            a = _ops.gatv2_attention_weights(*csr, xl, xr, att, stats, None, ctx.drop[0])
            ds = _ops.sparse_softmax_backward(*csr[:3], a, ga.reshape(a.shape))
            del a
            dxl2, dxr2, datt2 = _ops.gatv2_scores_backward(*a8, xl, xr, att, ds, ctx.drop[0])
            dxl += dxl2
            dxr += dxr2
            datt += datt2
        return (None,) * 8 + (dxl, dxr, datt, dxe, None, None, None, None)


def _head_slice(x, g0, hg):
    """Heads [g0, g0 + hg) of a (n, h, d) tensor as a contiguous (n, hg, d) tensor ((n, d) for one head: the one-head
    kernels and the fused passes take that form)."""
    part = x[:, g0:g0 + hg, :]
    return part.reshape(x.size(0), x.size(2)).contiguous() if hg == 1 else part.contiguous()


def _head_store(full, part, g0, hg):
    """full[:, g0 : g0 + hg, :] = part ((n, hg, d) or (n, d); the unfused SpMM returns zeros_like(x) rows: cut to full's)."""
    full[:, g0:g0 + hg, :].copy_(part[:full.size(0)].reshape(full.size(0), hg, full.size(2)))


def _bias_slice(b, g0, hg):
    """Heads [g0, g0 + hg) of the (E, h) score bias as a contiguous (E, hg) tensor ((E) for one head)"""
    part = b[:, g0:g0 + hg]
    return part.reshape(b.size(0)).contiguous() if hg == 1 else part.contiguous()


def _groups_forward(ctx, a8, Q, K, V, h, hg, drop=None, b=None):
    """The head-group loop of FusedAttention, FusedAttentionDropout (drop = (p, seed, offset)) and FusedAttentionBias
    (drop and the (E, h) score bias b): each group through _group_forward, its o written into the heads' slice; ctx
    keeps what the groups' backwards need."""
    import os
    mode = os.environ.get("GRAPHOP_FUSED_HEADS", FUSED_HEADS_MODE)
    ctx.groups = (h, hg, mode)
    o = Q.new_empty((Q.size(0),) + tuple(V.shape[1:]))
    kept = []
    for g0 in range(0, h, hg):
        Qg, Kg, Vg = (_head_slice(x, g0, hg) for x in (Q, K, V))
        og, keep = _group_forward(a8, Qg, Kg, Vg, mode, drop, g0, None if b is None else _bias_slice(b, g0, hg))
        _head_store(o, og, g0, hg)
        kept.append(keep)
        del Qg, Kg, Vg, og
    # per group: ("fused", o_g, stats_g) | ("keep", a_g) | ("recompute",) | ("drop", o_g, stats_g) | ("bias", o_g, stats_g)
    ctx.kept = kept
    ctx.save_for_backward(*a8, Q, K, V, *(() if b is None else (b,)))
    return o


def _groups_backward(ctx, a8, Q, K, V, dO, drop=None, b=None, need_db=True):
    """-> (dQ, dK, dV) of _groups_forward; with the score bias b -> (dQ, dK, dV, db), db (E, h) or None"""
    h, hg, mode = ctx.groups
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    db = torch.empty_like(b) if b is not None and need_db else None
    for gi, g0 in enumerate(range(0, h, hg)):
        Qg, Kg, Vg, dOg = (_head_slice(x, g0, hg) for x in (Q, K, V, dO))
        bg = None if b is None else _bias_slice(b, g0, hg)
        dQg, dKg, dVg, *dbg = _group_backward(a8, Qg, Kg, Vg, dOg, ctx.kept[gi], drop, g0, bg, need_db)
        for full, part in ((dQ, dQg), (dK, dKg), (dV, dVg)):
            _head_store(full, part, g0, hg)
        if db is not None:
            db[:, g0:g0 + hg].copy_(dbg[0].reshape(db.size(0), hg))
        del Qg, Kg, Vg, dOg, dQg, dKg, dVg, bg, dbg
    return (dQ, dK, dV) if b is None else (dQ, dK, dV, db)


def _group_forward(a8, Qg, Kg, Vg, mode, drop=None, head0=0, bg=None):
    """One head group's forward -> (o_g, what its backward needs).  drop = (p, seed, offset) with p > 0: the group through
    attention_dropout_forward as the heads head0 .. head0 + hg - 1 of the whole call; with the group's score bias bg
    (drop given, any p): through attention_bias_forward."""
    row, indptr_r, eid_r, indices_r = a8[:4]
    if bg is not None:
        og, stats = _ops.attention_bias_forward(row, indptr_r, eid_r, indices_r, Qg, Kg, Vg, bg, *drop, head0)
        return og, ("bias", og, stats)
    if drop is not None:
        og, stats = _ops.attention_dropout_forward(row, indptr_r, eid_r, indices_r, Qg, Kg, Vg, *drop, head0)
        return og, ("drop", og, stats)
    if _ops.attention_backward_is_fused(*a8, Qg, Kg) or Kg.size(0) < Qg.size(0):      # (as in FusedAttention.forward)
        og, stats = _ops.attention_forward(row, indptr_r, eid_r, indices_r, Qg, Kg, Vg)
        return og, ("fused", og, stats)
    s = _ops.maskedmm_csr_forward(row, indptr_r, eid_r, indices_r, Qg, Kg)
    a = _ops.sparse_softmax_forward(row, indptr_r, eid_r, s)
    del s
    og = _ops.vector_spmm_forward(row, indptr_r, eid_r, indices_r, a, Vg)
    return og, (("keep", a) if mode != "recompute" else ("recompute",))


def _group_backward(a8, Qg, Kg, Vg, dOg, kept, drop=None, head0=0, bg=None, need_db=True):
    row, indptr_r, eid_r, indices_r = a8[:4]
    if kept[0] == "bias":
        return _ops.attention_bias_backward(*a8, Qg, Kg, Vg, bg, kept[1], kept[2], dOg, *drop, head0, need_db)
    if kept[0] == "drop":
        return _ops.attention_dropout_backward(*a8, Qg, Kg, Vg, kept[1], kept[2], dOg, *drop, head0)
    if kept[0] == "fused":
        return _ops.attention_backward(*a8, Qg, Kg, Vg, kept[1], kept[2], dOg)
    if kept[0] == "keep":
        a = kept[1]
    else:
        s = _ops.maskedmm_csr_forward(row, indptr_r, eid_r, indices_r, Qg, Kg)
        a = _ops.sparse_softmax_forward(row, indptr_r, eid_r, s)
        del s
    da, dVg = _ops.vector_spmm_backward(*a8, a, dOg, Vg)
    ds = _ops.sparse_softmax_backward(row, indptr_r, eid_r, a, da)
    del da, a
    dQg, dKg = _ops.maskedmm_csr_backward(*a8, Qg, Kg, ds)
    return dQg, dKg, dVg


def fused_attention_step(g, Q, K, V, dO):
    """The same fwd+bwd as attention_step through the fused op; returns o."""
    o = FusedAttention.apply(*g.csr_args(), Q, K, V)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return o


def fused_attention_dropout_step(g, Q, K, V, dO, p, seed, offset=0):
    """fused_attention_step with dropout on the attention weights, through FusedAttentionDropout; returns o (no E-sized
    tensor is kept, the mask included)."""
    o = FusedAttentionDropout.apply(*g.csr_args(), Q, K, V, p, seed, offset)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return o


def fused_attention_bias_step(g, Q, K, V, b, dO, p=0.0, seed=0, offset=0):
    """fused_attention_dropout_step with the per-edge score bias b, through FusedAttentionBias; returns o (nothing
    edge-sized is kept but b, and b.grad where b requires it)."""
    o = FusedAttentionBias.apply(*g.csr_args(), Q, K, V, b, p, seed, offset)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return o


def attention_bias_step(g, Q, K, V, b, dO, p=0.0, seed=0, offset=0):
    """The composed yardstick of fused_attention_bias_step: MaskedMMCSR -> s + b -> SparseSoftmax ->
    (* edge_dropout_mask) -> VectorSPMM; s, a, the mask and their product are (E, h) tensors kept for the backward.
    Same decisions for the same (p, seed, offset); returns (s, a, o) with s the biased scores and a the undropped
    weights."""
    args = g.csr_args()
    s = MaskedMMCSR.apply(*args, Q, K) + b
    a = SparseSoftmax.apply(g.row, g.ptr_r, g.eid_r, s)
    w = a
    if p > 0:
        h = 1 if Q.dim() == 2 else Q.size(1)
        w = a * _ops.edge_dropout_mask(g.row, g.ptr_r, g.eid_r, g.indices_r, h, p, seed, offset, a.dtype)
    o = VectorSPMM.apply(*args, w, V)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return s, a, o


def fused_attention_edge_step(g, Q, K, V, xe, dO, p=0.0, seed=0, offset=0):
    """fused_attention_dropout_step with the edge rows xe in key and value, through FusedAttentionEdge; returns o
    (nothing edge-sized is kept but xe, and xe.grad where xe requires it)."""
    o = FusedAttentionEdge.apply(*g.csr_args(), Q, K, V, xe, p, seed, offset)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return o


def attention_edge_step(g, Q, K, V, xe, dO, p=0.0, seed=0, offset=0):
    """The composed yardstick of fused_attention_edge_step, for tests and timing only: torch index_selects of Q, K and V
    by slot, + xe[eid], SparseSoftmax, (* edge_dropout_mask), a segment sum -- K[dst] + xe, V[dst] + xe and their
    products are (E, h, d) tensors kept for the backward.  The chunk list must name every slot.  Same decisions as the
    fused step for the same (p, seed, offset); returns (s, a, o) with s, a (E, h) by edge id, a the undropped weights."""
    shape = Q.shape
    h = 1 if Q.dim() == 2 else Q.size(1)
    q3, k3, v3, xe3 = (x.reshape(x.size(0), h, x.size(-1)) for x in (Q, K, V, xe))
    slot_row = torch.repeat_interleave(g.row, g.ptr_r[1:] - g.ptr_r[:-1])
    xs = xe3.index_select(0, g.eid_r)
    kx = k3.index_select(0, g.indices_r) + xs
    vx = v3.index_select(0, g.indices_r) + xs
    s_slot = (q3.index_select(0, slot_row) * kx).sum(-1)
    s = torch.zeros_like(s_slot).index_copy(0, g.eid_r, s_slot)
    a = SparseSoftmax.apply(g.row, g.ptr_r, g.eid_r, s)
    w = a
    if p > 0:
        w = a * _ops.edge_dropout_mask(g.row, g.ptr_r, g.eid_r, g.indices_r, h, p, seed, offset, a.dtype).reshape(a.shape)
    o = torch.zeros_like(q3).index_add(0, slot_row, w.index_select(0, g.eid_r).unsqueeze(-1) * vx).reshape(shape)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return s, a, o


def fused_attention_etype_step(g, Q, K, V, R, etype, dO, p=0.0, seed=0, offset=0):
    """fused_attention_edge_step for a categorical edge feature, through FusedAttentionEdgeType: the table R and the
    int32 types etype (by edge id) stand where xe = R[etype] would; returns o (nothing of size (E, h, d) exists, and
    R.grad where R requires it has R's shape)."""
    o = FusedAttentionEdgeType.apply(*g.csr_args(), Q, K, V, R, etype, p, seed, offset)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return o


def attention_etype_step(g, Q, K, V, R, etype, dO, p=0.0, seed=0, offset=0):
    """The composed yardstick of fused_attention_etype_step, for tests and timing only: attention_edge_step on the
    materialised R[etype.long()] under autograd, which index_adds the (E, h, d) gradient back into R.grad."""
    return attention_edge_step(g, Q, K, V, R.index_select(0, etype.long()), dO, p, seed, offset)


def fused_attention_tbias_step(g, Q, K, V, B, etype, dO, p=0.0, seed=0, offset=0):
    """fused_attention_bias_step for a categorical edge feature, through FusedAttentionTypeBias: the table B and the
    int32 types etype (by edge id) stand where b = B[etype] would; returns o (nothing of size (E, h) exists, and B.grad
    where B requires it has B's shape)."""
    o = FusedAttentionTypeBias.apply(*g.csr_args(), Q, K, V, B, etype, p, seed, offset)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return o


def attention_tbias_step(g, Q, K, V, B, etype, dO, p=0.0, seed=0, offset=0):
    """The composed yardstick of fused_attention_tbias_step, for tests and timing only: fused_attention_bias_step on the
    materialised B[etype.long()] under autograd, which index_adds the (E, h) gradient back into B.grad."""
    return fused_attention_bias_step(g, Q, K, V, B.index_select(0, etype.long()), dO, p, seed, offset)


def _backward_pairs(pairs):
    """backward of the outputs whose gradient is given: pairs of (output, gradient or None)"""
    outs = [(t, g) for t, g in pairs if g is not None]
    if outs:
        torch.autograd.backward([t for t, _ in outs], [g for _, g in outs])


def fused_attention_weights_step(g, Q, K, V, dO, ga=None, b=None, xe=None, p=0.0, seed=0, offset=0):
    """The fused step that also returns its attention weights, through FusedAttentionWeights: backward of
    <o, dO> + <a, ga> (either gradient may be None; ga needs the plain or the bias mode); returns (o, a)."""
    o, a = FusedAttentionWeights.apply(*g.csr_args(), Q, K, V, b, xe, p, seed, offset)
    _backward_pairs(((o, dO), (a, ga)))
    _lib.check_errors(sync=False)     # as in attention_step
    return o, a


def attention_weights_step(g, Q, K, V, dO, ga=None, b=None, xe=None, p=0.0, seed=0, offset=0):
    """The composed yardstick of fused_attention_weights_step, for tests and timing only: the unfused ops (torch gathers
    with xe, as attention_edge_step: (E, h, d) temporaries, the chunk list must name every slot), a from SparseSoftmax --
    a second softmax with its own statistics -- and autograd through everything, the ga term included in every mode.
    Same decisions for the same (p, seed, offset); returns (s, a, o) with s, a by edge id, a the undropped weights."""
    args = g.csr_args()
    h = 1 if Q.dim() == 2 else Q.size(1)
    if xe is not None:
        q3, k3, v3, xe3 = (x.reshape(x.size(0), h, x.size(-1)) for x in (Q, K, V, xe))
        slot_row = torch.repeat_interleave(g.row, g.ptr_r[1:] - g.ptr_r[:-1])
        xs = xe3.index_select(0, g.eid_r)
        kx = k3.index_select(0, g.indices_r) + xs
        vx = v3.index_select(0, g.indices_r) + xs
        s_slot = (q3.index_select(0, slot_row) * kx).sum(-1)
        s = torch.zeros_like(s_slot).index_copy(0, g.eid_r, s_slot)
        if Q.dim() == 2:
            s = s.reshape(-1)
    else:
        s = MaskedMMCSR.apply(*args, Q, K)
        if b is not None:
            s = s + b
    a = SparseSoftmax.apply(g.row, g.ptr_r, g.eid_r, s)
    w = a
    if p > 0:
        w = a * _ops.edge_dropout_mask(g.row, g.ptr_r, g.eid_r, g.indices_r, h, p, seed, offset, a.dtype).reshape(a.shape)
    if xe is not None:
        o = torch.zeros_like(q3).index_add(0, slot_row, w.reshape(-1, h).index_select(0, g.eid_r).unsqueeze(-1) * vx)
        o = o.reshape(Q.shape)
    else:
        o = VectorSPMM.apply(*args, w, V)
        if o.size(0) != Q.size(0):          # the unfused SpMM returns zeros_like(x) rows
            o = o[:Q.size(0)]
    _backward_pairs(((o, dO), (a, ga)))
    _lib.check_errors(sync=False)     # as in attention_step
    return s, a, o


def fused_gat_attention_weights_step(g, el, er, V, dO, ga=None, ee=None, negative_slope=0.2, p=0.0, seed=0, offset=0):
    """The fused GAT step that also returns its attention weights, through FusedGATAttentionWeights: backward of
    <o, dO> + <a, ga> (either gradient may be None); returns (o, a).  The composed yardsticks are gat_attention_step,
    gat_attention_dropout_step and gat_edge_attention_step, which return a already."""
    o, a = FusedGATAttentionWeights.apply(*g.csr_args(), el, er, V, ee, negative_slope, p, seed, offset)
    _backward_pairs(((o, dO), (a, ga)))
    _lib.check_errors(sync=False)     # as in attention_step
    return o, a


def fused_gatv2_attention_weights_step(g, xl, xr, att, dO, ga=None, xe=None, negative_slope=0.2, p=0.0, seed=0,
                                       offset=0):
    """The fused GATv2 step that also returns its attention weights, through FusedGATv2AttentionWeights: backward of
    <o, dO> + <a, ga> (either gradient may be None; ga needs xe=None); returns (o, a).  The composed yardsticks are
    gatv2_attention_step, gatv2_attention_dropout_step and gatv2_edge_attention_step, which return a already."""
    o, a = FusedGATv2AttentionWeights.apply(*g.csr_args(), xl, xr, att, xe, negative_slope, p, seed, offset)
    _backward_pairs(((o, dO), (a, ga)))
    _lib.check_errors(sync=False)     # as in attention_step
    return o, a


def attention_dropout_step(g, Q, K, V, dO, p, seed, offset=0):
    """attention_step with dropout on the attention weights, composed: MaskedMMCSR -> SparseSoftmax ->
    (* edge_dropout_mask) -> VectorSPMM; a, the mask and their product are (E, h) tensors kept for the backward.  Same
    decisions as fused_attention_dropout_step for the same (p, seed, offset); returns (s, a, o) with a the undropped
    weights."""
    args = g.csr_args()
    s = MaskedMMCSR.apply(*args, Q, K)
    a = SparseSoftmax.apply(g.row, g.ptr_r, g.eid_r, s)
    h = 1 if Q.dim() == 2 else Q.size(1)
    mask = _ops.edge_dropout_mask(g.row, g.ptr_r, g.eid_r, g.indices_r, h, p, seed, offset, a.dtype)
    o = VectorSPMM.apply(*args, a * mask, V)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return s, a, o


def attention_step(g, Q, K, V, dO):
    """One fwd+bwd of the composed hot path the headline metric times:
    s = SDDMM(Q, K); a = row-softmax(s); o = SpMM(a, V); o.backward(dO).
    Q, K, V must be leaf tensors with requires_grad; returns (s, a, o)."""
    args = g.csr_args()
    s = MaskedMMCSR.apply(*args, Q, K)
    a = SparseSoftmax.apply(g.row, g.ptr_r, g.eid_r, s)
    o = VectorSPMM.apply(*args, a, V)
    o.backward(dO)
    # a device-side abort (include/graphop_hip.h: graphop_check_device_errors) of a launch that has already finished is
    # raised HERE, before the gradients leave the step; one still in flight is sticky and fails the next op call
    _lib.check_errors(sync=False)
    return s, a, o


def gat_attention_step(g, el, er, V, dO, negative_slope=0.2):
    """One fwd+bwd of GAT-style additive attention, the counterpart of attention_step:
    s = LeakyReLU(el[i] + er[j]); a = row-softmax(s); o = SpMM(a, V); o.backward(dO).
    el, er, V must be leaf tensors with requires_grad; returns (s, a, o)."""
    args = g.csr_args()
    s = GATScores.apply(*args, el, er, negative_slope)
    a = SparseSoftmax.apply(g.row, g.ptr_r, g.eid_r, s)
    o = VectorSPMM.apply(*args, a, V)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return s, a, o


def gatv2_attention_step(g, xl, xr, att, dO, negative_slope=0.2, V=None):
    """One fwd+bwd of GATv2 attention, the counterpart of gat_attention_step:
    s = att . LeakyReLU(xl[i] + xr[j]); a = row-softmax(s); o = SpMM(a, V); o.backward(dO).
    V=None aggregates xr itself (the GATv2Conv convention: the transformed neighbour features serve both the score and
    the message; autograd then sums the two gradients into xr).  xl, xr, att (and V) must be leaf tensors with
    requires_grad; returns (s, a, o)."""
    args = g.csr_args()
    s = GATv2Scores.apply(*args, xl, xr, att, negative_slope)
    a = SparseSoftmax.apply(g.row, g.ptr_r, g.eid_r, s)
    o = VectorSPMM.apply(*args, a, xr if V is None else V)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return s, a, o


def fused_gatv2_attention_step(g, xl, xr, att, dO, negative_slope=0.2):
    """The counterpart of gatv2_attention_step(V=None) through FusedGATv2Attention: o = GATv2 layer(xl, xr, att);
    o.backward(dO).  xl, xr, att must be leaf tensors with requires_grad; returns o (no E-sized tensor is kept or made)."""
    o = FusedGATv2Attention.apply(*g.csr_args(), xl, xr, att, negative_slope)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return o


def fused_gat_attention_step(g, el, er, V, dO, negative_slope=0.2):
    """The counterpart of gat_attention_step through FusedGATAttention: o = GAT layer(el, er, V); o.backward(dO).
    el, er, V must be leaf tensors with requires_grad; returns o (no E-sized tensor is kept or made)."""
    o = FusedGATAttention.apply(*g.csr_args(), el, er, V, negative_slope)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return o


def gat_attention_dropout_step(g, el, er, V, dO, p, seed, offset=0, negative_slope=0.2):
    """gat_attention_step with dropout on the attention weights, composed: GATScores -> SparseSoftmax ->
    (* edge_dropout_mask) -> VectorSPMM; the mask is one more (E, h) tensor kept for the backward.  Same decisions as
    fused_gat_attention_dropout_step for the same (p, seed, offset); returns (s, a, o) with a the undropped weights."""
    args = g.csr_args()
    s = GATScores.apply(*args, el, er, negative_slope)
    a = SparseSoftmax.apply(g.row, g.ptr_r, g.eid_r, s)
    h = 1 if el.dim() == 1 else el.size(1)
    mask = _ops.edge_dropout_mask(g.row, g.ptr_r, g.eid_r, g.indices_r, h, p, seed, offset, a.dtype)
    o = VectorSPMM.apply(*args, a * mask, V)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return s, a, o


def fused_gat_attention_dropout_step(g, el, er, V, dO, p, seed, offset=0, negative_slope=0.2):
    """The counterpart of gat_attention_dropout_step through FusedGATAttentionDropout; returns o (no E-sized tensor is
    kept or made, the mask included)."""
    o = FusedGATAttentionDropout.apply(*g.csr_args(), el, er, V, negative_slope, p, seed, offset)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return o


def gatv2_attention_dropout_step(g, xl, xr, att, dO, p, seed, offset=0, negative_slope=0.2):
    """gatv2_attention_step(V=None) with dropout on the attention weights, composed: GATv2Scores -> SparseSoftmax ->
    (* edge_dropout_mask) -> VectorSPMM(., xr); the mask is one more (E, h) tensor kept for the backward.  Same decisions
    as fused_gatv2_attention_dropout_step for the same (p, seed, offset); returns (s, a, o) with a the undropped weights."""
    args = g.csr_args()
    s = GATv2Scores.apply(*args, xl, xr, att, negative_slope)
    a = SparseSoftmax.apply(g.row, g.ptr_r, g.eid_r, s)
    h = 1 if xl.dim() == 2 else xl.size(1)
    mask = _ops.edge_dropout_mask(g.row, g.ptr_r, g.eid_r, g.indices_r, h, p, seed, offset, a.dtype)
    o = VectorSPMM.apply(*args, a * mask, xr)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return s, a, o


def fused_gatv2_attention_dropout_step(g, xl, xr, att, dO, p, seed, offset=0, negative_slope=0.2):
    """The counterpart of gatv2_attention_dropout_step through FusedGATv2AttentionDropout; returns o (no E-sized tensor
    is kept or made, the mask included)."""
    o = FusedGATv2AttentionDropout.apply(*g.csr_args(), xl, xr, att, negative_slope, p, seed, offset)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return o


def gat_edge_attention_step(g, el, er, ee, V, dO, negative_slope=0.2, p=0.0, seed=0, offset=0):
    """One fwd+bwd of GAT attention with a per-edge score term, composed from the unfused ops:
    z = el[i] + er[j] (GATScores at slope 1) + ee; s = LeakyReLU(z); a = row-softmax(s); (* edge_dropout_mask when
    p > 0); o = SpMM(a, V); o.backward(dO).  Keeps z, z + ee, s and a (and the mask) as (E, h) tensors.  el, er, V must
    be leaf tensors with requires_grad; returns (s, a, o) with a the undropped weights."""
    args = g.csr_args()
    z = GATScores.apply(*args, el, er, 1.0) + ee
    s = torch.nn.functional.leaky_relu(z, negative_slope)
    a = SparseSoftmax.apply(g.row, g.ptr_r, g.eid_r, s)
    w = a
    if p > 0:
        h = 1 if el.dim() == 1 else el.size(1)
        w = a * _ops.edge_dropout_mask(g.row, g.ptr_r, g.eid_r, g.indices_r, h, p, seed, offset, a.dtype)
    o = VectorSPMM.apply(*args, w, V)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return s, a, o


def fused_gat_edge_attention_step(g, el, er, ee, V, dO, negative_slope=0.2, p=0.0, seed=0, offset=0):
    """The counterpart of gat_edge_attention_step through FusedGATEdgeAttention; returns o.  The gradient of ee is the
    only edge-sized tensor made, and none is when ee does not require grad."""
    o = FusedGATEdgeAttention.apply(*g.csr_args(), el, er, ee, V, negative_slope, p, seed, offset)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return o


def gatv2_edge_attention_step(g, xl, xr, xe, att, dO, negative_slope=0.2, p=0.0, seed=0, offset=0):
    """One fwd+bwd of GATv2 attention with edge features, composed: the score in plain torch (index_select of xl and xr
    over the row-major slots, + xe[eid], leaky_relu, (. * att).sum(-1), put back in edge-id order), then SparseSoftmax,
    (* edge_dropout_mask when p > 0) and VectorSPMM(., xr); o.backward(dO).  Keeps xl[src], xr[dst], z and LeakyReLU(z)
    as (E, h, d) tensors and s, a (and the mask) as (E, h) ones.  The operands that need a gradient must be leaf tensors
    with requires_grad; returns (s, a, o) with a the undropped weights."""
    z = (xl.index_select(0, g.src) + xr.index_select(0, g.dst)) + xe.index_select(0, g.eid_r)
    s_slot = (torch.nn.functional.leaky_relu(z, negative_slope) * att).sum(-1)
    s = torch.zeros((g.n_edges,) + tuple(s_slot.shape[1:]), dtype=s_slot.dtype,
                    device=s_slot.device).index_copy(0, g.eid_r, s_slot)
    a = SparseSoftmax.apply(g.row, g.ptr_r, g.eid_r, s)
    w = a
    if p > 0:
        h = 1 if xl.dim() == 2 else xl.size(1)
        w = a * _ops.edge_dropout_mask(g.row, g.ptr_r, g.eid_r, g.indices_r, h, p, seed, offset, a.dtype)
    o = VectorSPMM.apply(*g.csr_args(), w, xr)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return s, a, o


def fused_gatv2_edge_attention_step(g, xl, xr, xe, att, dO, negative_slope=0.2, p=0.0, seed=0, offset=0):
    """The counterpart of gatv2_edge_attention_step through FusedGATv2EdgeAttention; returns o.  The gradient of xe is the
    only edge-sized tensor made, and none is when xe does not require grad."""
    o = FusedGATv2EdgeAttention.apply(*g.csr_args(), xl, xr, xe, att, negative_slope, p, seed, offset)
    o.backward(dO)
    _lib.check_errors(sync=False)     # as in attention_step
    return o
