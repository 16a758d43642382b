"""The reference's operator surface, MI355X-native.

Mirror of the pybind11 module ``graphop`` (``graphop/graphop.cpp:216-225``): the same eight
names, positional signatures, return types (a Tensor, or a list of two Tensors), output shapes
(``(e)`` when h == 1 else ``(e, h)``, ``graphop_kernel.cu:284``) and error behaviour
(``RuntimeError("<arg> must be a CUDA tensor")`` / ``"<arg> must be contiguous"``,
``graphop.cpp:4-6``).  Each function flattens its tensors to pointers + sizes and calls the C ABI
of ``libgraphop_hip.so`` (``include/graphop_hip.h``) on the current stream, without syncing.

Additionally every op is registered as ``torch.ops.graphop.<name>`` (the reference has no
TORCH_LIBRARY registration; BASELINE.json's north_star asks for this surface).

Deliberate, documented deviations from the reference:
  * ``dy`` is made contiguous in the backward ops (the reference forgets to check it,
    ``graphop.cpp:120-129`` and reads garbage from a strided ``dy``).
  * graphs are validated once per (row, indptr, eid, indices) identity when their plan is built
    (index range, indptr bounds): the reference reads out of bounds instead.
  * ``vector_spmm_backward`` processes every column chunk (reference grid bug,
    ``graphop_kernel.cu:566,588``).
  * non-square operands are allowed: B / x may have a different row count than A / y.
"""
import torch

from . import _lib
from ._lib import check, dtype_code, get_plan, lib, ptr, stream_of

__all__ = ["maskedmm_csr_forward", "maskedmm_csr_backward", "node_mul_edge_forward",
           "node_mul_edge_backward", "sparse_softmax_forward", "sparse_softmax_backward",
           "vector_spmm_forward", "vector_spmm_backward"]
# extra ops (not in the reference's module): the fused attention step, SURVEY.md 8f N2, and its form with attention
# dropout (attention_dropout_forward / _backward) and with a per-edge score bias (attention_bias_forward /
# _backward) and with edge features in key and value (attention_edge_forward / _backward),
# the attention weights of all of these from the row statistics they return (attention_weights),
# the edge-feature form for a categorical feature: a table and an int32 type per edge (attention_etype_*),
# the score bias for a categorical feature: a scalar per (type, head) and the same int32 (attention_tbias_*),
# the GAT additive attention scores (LeakyReLU(el[i] + er[j]) per edge and head), the fused GAT attention layer and
# its forms with attention dropout (plus the mask they apply, as an edge tensor, for the composed path), and the GATv2
# scores (att . LeakyReLU(xl[i] + xr[j]) per edge and head), and the fused GAT layer with a per-edge score term
# (LeakyReLU(el[i] + er[j] + ee[e]), GATConv(edge_dim=...) / EGATConv), and the fused GATv2 layer with edge features
# (att . LeakyReLU(xl[i] + xr[j] + xe[e]), GATv2Conv(edge_dim=...)): the optional xe / need_dxe arguments of the two
# gatv2_attention_dropout_* ops, and the attention weights of the six fused GAT / GATv2 layers from the row statistics
# they return (gat_attention_weights, gatv2_attention_weights).  EXTRA_OPS lists them, below _SCHEMAS.

_NULL = None
# the index arrays of a call by argument name: one CSR orientation without and with `indices`, and the two spellings
# of the backward ops' second orientation
_CSR3 = ("row", "indptr", "eid")
_CSR = _CSR3 + ("indices",)
_CSR_RC = ("row", "indptr_r", "eid_r", "indices_r", "col", "indptr_c", "eid_c", "indices_c")
_CSR_T = _CSR + ("col", "indptr_t", "eid_t", "indices_t")


def _check_input(t, name):
    # CHECK_CUDA / CHECK_CONTIGUOUS, graphop.cpp:4-6
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)


def _check_index(t, name):
    if t.dtype != torch.int64:
        # the reference throws from .data<int64_t>() (graphop_kernel.cu:293)
        raise RuntimeError("expected scalar type Long but found %s (%s)" % (t.dtype, name))


def _check_csr(tensors, names, *values):
    """CHECK_INPUT on the index arrays `tensors`, called `names`, and on the value operands, given as (tensor, name)
    pairs; then CHECK_INDEX on the index arrays."""
    for t, n in zip(tensors, names):
        _check_input(t, n)
    for t, n in values:
        _check_input(t, n)
    for t, n in zip(tensors, names):
        _check_index(t, n)


def _check_grad(t, name):
    # CHECK_CUDA alone: a gradient is made contiguous, not refused
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)


def _check_edge_rows(t, name, n_edges):
    # the C ABI takes a raw pointer plus n_edges: fewer rows than edge ids would be read (or written) out of bounds
    if t.dim() < 1 or t.size(0) < n_edges:
        raise RuntimeError("%s must hold one entry per edge id: %d rows for %d edges" % (name, t.size(0), n_edges))


def _edge_out(e, h, dtype, device):
    return torch.empty((e,) if h == 1 else (e, h), dtype=dtype, device=device)     # graphop_kernel.cu:284


def _same_dtype(a, b, na, nb):
    if a.dtype != b.dtype:
        raise RuntimeError("expected %s and %s to have the same dtype, got %s and %s"
                           % (na, nb, a.dtype, b.dtype))


def maskedmm_csr_forward(row, indptr, eid, indices, A, B):
    """y[eid[j], k] = <A[row[c], k], B[indices[j], k]>   (graphop.cpp:16-30)"""
    _check_csr((row, indptr, eid, indices), _CSR, (A, "A"), (B, "B"))
    _same_dtype(A, B, "A", "B")
    e, d = eid.size(0), A.size(-1)
    h = 1 if A.dim() == 2 else A.size(1)                    # graphop_kernel.cu:283
    y = _edge_out(e, h, A.dtype, A.device)
    with _lib.device_guard(A.device):
        plan = get_plan(row, indptr, eid, indices, B.size(0))
        check(lib().graphop_maskedmm_csr_forward(
            dtype_code(A), ptr(row), ptr(indptr), ptr(eid), ptr(indices), ptr(A), ptr(B), ptr(y),
            row.size(0), e, A.size(0), B.size(0), h, d, plan.handle, stream_of(A)))
    return y


def maskedmm_csr_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c,
                          A, B, dy):
    """-> [dA, dB]   (graphop.cpp:108-131)"""
    _check_csr((row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c), _CSR_RC, (A, "A"), (B, "B"))
    _check_grad(dy, "dy")
    _same_dtype(A, B, "A", "B")
    _same_dtype(A, dy, "A", "dy")
    dy = dy.contiguous()
    _check_edge_rows(dy, "dy", eid_r.size(0))
    d = A.size(-1)
    h = dy.size(1) if dy.dim() == 2 else 1                  # graphop_kernel.cu:373
    dA, dB = torch.empty_like(A), torch.empty_like(B)
    with _lib.device_guard(A.device):
        plan_r = get_plan(row, indptr_r, eid_r, indices_r, B.size(0))
        plan_c = get_plan(col, indptr_c, eid_c, indices_c, A.size(0))
        check(lib().graphop_maskedmm_csr_backward(
            dtype_code(A), ptr(row), ptr(indptr_r), ptr(eid_r), ptr(indices_r), ptr(col),
            ptr(indptr_c), ptr(eid_c), ptr(indices_c), ptr(A), ptr(B), ptr(dy), ptr(dA), ptr(dB),
            row.size(0), col.size(0), eid_r.size(0), A.size(0), B.size(0), h, d,
            plan_r.handle, plan_c.handle, stream_of(A)))
    return [dA, dB]


def sparse_softmax_forward(row, indptr, eid, x):
    """Per-row (per-head) softmax of edge values   (graphop.cpp:59-69)"""
    _check_csr((row, indptr, eid), _CSR3, (x, "x"))
    _check_edge_rows(x, "x", eid.size(0))
    h = x.size(1) if x.dim() == 2 else 1
    y = torch.empty_like(x)
    with _lib.device_guard(x.device):
        plan = get_plan(row, indptr, eid, None, 0)
        ws, ws_rows = None, 0
        if not plan.info.row_owned:                          # general layout: atomics + scratch
            ws_rows = plan.info.max_row + 1
            ws = torch.empty(2 * ws_rows * h, dtype=x.dtype, device=x.device)
        check(lib().graphop_sparse_softmax_forward(
            dtype_code(x), ptr(row), ptr(indptr), ptr(eid), ptr(x), ptr(y), row.size(0),
            eid.size(0), h, ptr(ws), ws_rows, plan.handle, stream_of(x)))
    return y


def sparse_softmax_backward(row, indptr, eid, y, dy):
    """dx = dy*y - (sum_row dy*y)*y   (graphop.cpp:163-175)"""
    _check_csr((row, indptr, eid), _CSR3, (y, "y"))
    _check_grad(dy, "dy")
    _same_dtype(y, dy, "y", "dy")
    dy = dy.contiguous()
    _check_edge_rows(y, "y", eid.size(0))
    _check_edge_rows(dy, "dy", eid.size(0))
    h = dy.size(1) if dy.dim() == 2 else 1
    dx = torch.empty_like(dy)
    with _lib.device_guard(y.device):
        plan = get_plan(row, indptr, eid, None, 0)
        ws, ws_rows = None, 0
        if not plan.info.row_owned:
            ws_rows = plan.info.max_row + 1
            ws = torch.empty(ws_rows * h, dtype=y.dtype, device=y.device)
        check(lib().graphop_sparse_softmax_backward(
            dtype_code(y), ptr(row), ptr(indptr), ptr(eid), ptr(y), ptr(dy), ptr(dx), row.size(0),
            eid.size(0), h, ptr(ws), ws_rows, plan.handle, stream_of(y)))
    return dx


def vector_spmm_forward(row, indptr, eid, indices, edata, x):
    """y[row[c], k] += sum_j edata[eid[j], k] * x[indices[j], k]   (graphop.cpp:79-93)"""
    _check_csr((row, indptr, eid, indices), _CSR, (edata, "edata"), (x, "x"))
    _same_dtype(edata, x, "edata", "x")
    _check_edge_rows(edata, "edata", eid.size(0))
    h = edata.size(1) if edata.dim() == 2 else 1            # graphop_kernel.cu:520
    d = x.size(-1)
    y = torch.empty_like(x)                                  # zeros_like(x), :527
    with _lib.device_guard(x.device):
        plan = get_plan(row, indptr, eid, indices, x.size(0))
        if plan.info.max_row >= x.size(0):
            raise RuntimeError("vector_spmm_forward: row id %d but y = zeros_like(x) has %d rows"
                               % (plan.info.max_row, x.size(0)))
        check(lib().graphop_vector_spmm_forward(
            dtype_code(x), ptr(row), ptr(indptr), ptr(eid), ptr(indices), ptr(edata), ptr(x),
            ptr(y), row.size(0), eid.size(0), x.size(0), x.size(0), h, d, plan.handle,
            stream_of(x)))
    return y


def vector_spmm_backward(row, indptr, eid, indices, col, indptr_t, eid_t, indices_t, edata, dy, x):
    """-> [dedata, dx]; NB ``dy`` comes before ``x``   (graphop.cpp:190-214)"""
    _check_csr((row, indptr, eid, indices, col, indptr_t, eid_t, indices_t), _CSR_T,
               (edata, "edata"), (dy, "dy"), (x, "x"))
    _same_dtype(edata, x, "edata", "x")
    _same_dtype(dy, x, "dy", "x")
    _check_edge_rows(edata, "edata", eid.size(0))
    h = edata.size(1) if edata.dim() == 2 else 1            # graphop_kernel.cu:560
    d = x.size(-1)
    dedata, dx = torch.empty_like(edata), torch.empty_like(x)
    with _lib.device_guard(x.device):
        plan_r = get_plan(row, indptr, eid, indices, x.size(0))
        plan_c = get_plan(col, indptr_t, eid_t, indices_t, dy.size(0))
        if plan_c.info.max_row >= x.size(0):
            raise RuntimeError("vector_spmm_backward: col id %d but dx has %d rows"
                               % (plan_c.info.max_row, x.size(0)))
        check(lib().graphop_vector_spmm_backward(
            dtype_code(x), ptr(row), ptr(indptr), ptr(eid), ptr(indices), ptr(col), ptr(indptr_t),
            ptr(eid_t), ptr(indices_t), ptr(edata), ptr(dy), ptr(x), ptr(dedata), ptr(dx),
            row.size(0), col.size(0), eid.size(0), x.size(0), dy.size(0), h, d, plan_r.handle,
            plan_c.handle, stream_of(x)))
    return [dedata, dx]


def node_mul_edge_forward(row, indptr, eid, A, B):
    """y[eid[j], k] = <A[row[c], k], B[eid[j]]>   (graphop.cpp:39-51)"""
    _check_csr((row, indptr, eid), _CSR3, (A, "A"), (B, "B"))
    _same_dtype(A, B, "A", "B")
    e, d = eid.size(0), A.size(-1)
    h = 1 if A.dim() == 2 else A.size(1)
    if B.size(0) < e or B.size(-1) != d:
        raise RuntimeError("node_mul_edge_forward: B must be (n_edges, d)")
    y = _edge_out(e, h, A.dtype, A.device)
    with _lib.device_guard(A.device):
        plan = get_plan(row, indptr, eid, None, 0)
        check(lib().graphop_node_mul_edge_forward(
            dtype_code(A), ptr(row), ptr(indptr), ptr(eid), ptr(A), ptr(B), ptr(y), row.size(0), e,
            A.size(0), h, d, plan.handle, stream_of(A)))
    return y


def node_mul_edge_backward(row, indptr, eid, A, B, dy):
    """-> [dA, dB]   (graphop.cpp:141-154)"""
    _check_csr((row, indptr, eid), _CSR3, (A, "A"), (B, "B"))
    _check_grad(dy, "dy")
    _same_dtype(A, B, "A", "B")
    _same_dtype(A, dy, "A", "dy")
    dy = dy.contiguous()
    e = eid.size(0)
    _check_edge_rows(dy, "dy", e)
    d = A.size(-1)
    h = dy.size(1) if dy.dim() == 2 else 1
    if B.size(0) != e or B.size(-1) != d:
        raise RuntimeError("node_mul_edge_backward: B must be (n_edges, d)")
    dA, dB = torch.empty_like(A), torch.empty_like(B)
    with _lib.device_guard(A.device):
        plan = get_plan(row, indptr, eid, None, 0)
        check(lib().graphop_node_mul_edge_backward(
            dtype_code(A), ptr(row), ptr(indptr), ptr(eid), ptr(A), ptr(B), ptr(dy), ptr(dA),
            ptr(dB), row.size(0), e, A.size(0), h, d, plan.handle, stream_of(A)))
    return [dA, dB]


# ---- fused attention step (extra op; the composition wrapper.py:20-30, 8-18, 44-55) ------------------
def _workspace(like, dtype, backward, e, n_q, n_k, h, d, plan_r, plan_c, dropout=False, bias=None):
    """bias: None, or whether the call with a score bias is a backward that writes db"""
    import ctypes
    nbytes = ctypes.c_int64(0)
    query = lib().graphop_attention_dropout_workspace_bytes if dropout else lib().graphop_attention_workspace_bytes
    extra = ()
    if bias is not None:
        query, extra = lib().graphop_attention_bias_workspace_bytes, (1 if bias else 0,)
    check(query(
        dtype, 1 if backward else 0, e, n_q, n_k, h, d, plan_r.handle if plan_r is not None else _NULL,
        plan_c.handle if plan_c is not None else _NULL, stream_of(like), *extra, ctypes.byref(nbytes)))
    return torch.empty(max(1, nbytes.value), dtype=torch.uint8, device=like.device), nbytes.value


def attention_backward_is_fused(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K):
    """True when attention_backward will run its fused window passes for this graph and these
    shapes (fp32, one head, sweepable plans, tables beyond the L2), its chunk-driver passes, or -- several
    heads of a supported (h, d), DESIGN.md 4.5l -- the several-head passes; False when it would compose
    the unfused ops, recomputing s and a."""
    import ctypes
    d = Q.size(-1)
    h = 1 if Q.dim() == 2 else Q.size(1)
    out = ctypes.c_int(0)
    with _lib.device_guard(Q.device):
        plan_r = get_plan(row, indptr_r, eid_r, indices_r, K.size(0))
        plan_c = get_plan(col, indptr_c, eid_c, indices_c, Q.size(0))
        check(lib().graphop_attention_backward_is_fused(dtype_code(Q), eid_r.size(0), Q.size(0), K.size(0), h, d,
                                                        plan_r.handle, plan_c.handle, stream_of(Q), ctypes.byref(out)))
    return bool(out.value)


def _attn_bias(fn, b, Q, n_edges, h):
    """b checked against the graph and the heads: (n_edges) for 2-D Q / K / V, else (n_edges, h), in Q's dtype"""
    _same_dtype(Q, b, "Q", "b")
    _check_edge_rows(b, "b", n_edges)
    if tuple(b.shape) != ((n_edges,) if Q.dim() == 2 else (n_edges, h)):
        raise RuntimeError("%s: b must be (n_edges) for 2-D Q / K / V, else (n_edges, h) with n_edges = %d and h = %d, "
                           "got b %s, Q %s" % (fn, n_edges, h, tuple(b.shape), tuple(Q.shape)))


def _attention_forward(fn, row, indptr, eid, indices, Q, K, V, drop=(), b=None):
    """attention_forward (drop = ()), attention_dropout_forward (drop = (p, seed, offset, head0)) or, with the score
    bias b, attention_bias_forward as `fn`"""
    _check_csr((row, indptr, eid, indices), _CSR, (Q, "Q"), (K, "K"), (V, "V"), *(((b, "b"),) if b is not None else ()))
    _same_dtype(Q, K, "Q", "K")
    _same_dtype(Q, V, "Q", "V")
    if K.shape != V.shape or Q.shape[1:] != K.shape[1:]:
        raise RuntimeError("%s: Q (n_q,[h,]d), K and V (n_k,[h,]d) expected" % fn)
    e, d = eid.size(0), Q.size(-1)
    h = 1 if Q.dim() == 2 else Q.size(1)
    n_q, n_k = Q.size(0), K.size(0)
    bias = ()
    if b is not None:
        _attn_bias(fn, b, Q, e, h)
        bias = (ptr(b),)
    o = torch.empty_like(Q)
    stats = torch.empty((n_q, h, 2), dtype=Q.dtype, device=Q.device)
    with _lib.device_guard(Q.device):
        plan = get_plan(row, indptr, eid, indices, n_k)
        ws, nbytes = _workspace(Q, dtype_code(Q), False, e, n_q, n_k, h, d, plan, None, bool(drop),
                                False if b is not None else None)
        check(getattr(lib(), "graphop_" + fn)(
            dtype_code(Q), ptr(row), ptr(indptr), ptr(eid), ptr(indices), ptr(Q), ptr(K), ptr(V), *bias,
            ptr(o), ptr(stats), row.size(0), e, n_q, n_k, h, d, ptr(ws), nbytes, plan.handle,
            stream_of(Q), *drop))
    return [o, stats]


def attention_forward(row, indptr, eid, indices, Q, K, V):
    """-> [o, stats]: o = vector_spmm(sparse_softmax(maskedmm_csr(Q, K)), V) over the row-major CSR,
    without returning the E-sized s / a.  stats (n_q, h, 2) = (row max, 1 / sum exp) is what
    attention_backward needs to recompute them."""
    return _attention_forward("attention_forward", row, indptr, eid, indices, Q, K, V)


def _attention_backward(fn, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c,
                        Q, K, V, o, stats, dO, drop=(), b=None, need_db=True):
    """attention_backward (drop = ()), attention_dropout_backward (drop = (p, seed, offset, head0)) or, with the score
    bias b, attention_bias_backward as `fn`: then -> [dQ, dK, dV, db], db an empty (0,) tensor with need_db=False"""
    _check_csr((row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c), _CSR_RC,
               (Q, "Q"), (K, "K"), (V, "V"), *(((b, "b"),) if b is not None else ()), (o, "o"), (stats, "stats"))
    _check_grad(dO, "dO")
    for t, n in ((K, "K"), (V, "V"), (o, "o"), (stats, "stats"), (dO, "dO")):
        _same_dtype(Q, t, "Q", n)
    dO = dO.contiguous()
    e, d = eid_r.size(0), Q.size(-1)
    h = 1 if Q.dim() == 2 else Q.size(1)
    n_q, n_k = Q.size(0), K.size(0)
    if o.shape != Q.shape or dO.shape != Q.shape or stats.numel() != n_q * h * 2:
        raise RuntimeError("%s: o, dO must match Q and stats must be (n_q, h, 2)" % fn)
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    if b is not None:
        _attn_bias(fn, b, Q, e, h)
    with _lib.device_guard(Q.device):
        plan_r = get_plan(row, indptr_r, eid_r, indices_r, n_k)
        plan_c = get_plan(col, indptr_c, eid_c, indices_c, n_q)
        bias = dbias = ()
        if b is not None:
            # db[e] is written once per row-major slot: only a chunk list that leaves slots out needs the zeros
            db = (torch.empty_like(b) if plan_r.info.full_coverage else torch.zeros_like(b)) if need_db \
                else torch.empty((0,), dtype=b.dtype, device=b.device)
            bias, dbias = (ptr(b),), (ptr(db) if need_db else _NULL,)
        ws, nbytes = _workspace(Q, dtype_code(Q), True, e, n_q, n_k, h, d, plan_r, plan_c, bool(drop),
                                bool(need_db) if b is not None else None)
        check(getattr(lib(), "graphop_" + fn)(
            dtype_code(Q), ptr(row), ptr(indptr_r), ptr(eid_r), ptr(indices_r), ptr(col),
            ptr(indptr_c), ptr(eid_c), ptr(indices_c), ptr(Q), ptr(K), ptr(V), *bias, ptr(o), ptr(stats),
            ptr(dO), ptr(dQ), ptr(dK), ptr(dV), *dbias, row.size(0), col.size(0), e, n_q, n_k, h, d,
            ptr(ws), nbytes, plan_r.handle, plan_c.handle, stream_of(Q), *drop))
    return [dQ, dK, dV] if b is None else [dQ, dK, dV, db]


def attention_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c,
                       Q, K, V, o, stats, dO):
    """-> [dQ, dK, dV] of the fused step for the output gradient dO."""
    return _attention_backward("attention_backward", row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c,
                               Q, K, V, o, stats, dO)


# ---- GAT additive attention scores (extra op) ------------------------------------------------------------
def _gat_heads(el, er, fn):
    """h of the (n_src[, h]) / (n_dst[, h]) per-node score tables; they must agree in dtype and h."""
    _same_dtype(el, er, "el", "er")
    if el.dim() not in (1, 2) or er.dim() != el.dim() or (el.dim() == 2 and el.size(1) != er.size(1)):
        raise RuntimeError("%s: el (n_src[, h]) and er (n_dst[, h]) must have the same h, got %s and %s"
                           % (fn, tuple(el.shape), tuple(er.shape)))
    return 1 if el.dim() == 1 else el.size(1)


def gat_scores_forward(row, indptr, eid, indices, el, er, negative_slope=0.2):
    """y[eid[j], k] = LeakyReLU(el[row[c], k] + er[indices[j], k], negative_slope); y is (e) if h == 1 else (e, h)"""
    _check_csr((row, indptr, eid, indices), _CSR, (el, "el"), (er, "er"))
    h = _gat_heads(el, er, "gat_scores_forward")
    e = eid.size(0)
    y = _edge_out(e, h, el.dtype, el.device)
    with _lib.device_guard(el.device):
        plan = get_plan(row, indptr, eid, indices, er.size(0))
        check(lib().graphop_gat_scores_forward(
            dtype_code(el), ptr(row), ptr(indptr), ptr(eid), ptr(indices), ptr(el), ptr(er), ptr(y), row.size(0), e,
            el.size(0), er.size(0), h, float(negative_slope), plan.handle, stream_of(el)))
    return y


def gat_scores_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, dy,
                        negative_slope=0.2):
    """-> [del, der] of gat_scores_forward for the score gradient dy (z is recomputed from el and er)"""
    _check_csr((row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c), _CSR_RC, (el, "el"), (er, "er"))
    _check_grad(dy, "dy")
    h = _gat_heads(el, er, "gat_scores_backward")
    _same_dtype(el, dy, "el", "dy")
    dy = dy.contiguous()
    e = eid_r.size(0)
    if dy.numel() != e * h:
        raise RuntimeError("gat_scores_backward: dy must hold (n_edges, h) = (%d, %d) values, got %s"
                           % (e, h, tuple(dy.shape)))
    d_el, d_er = torch.empty_like(el), torch.empty_like(er)
    with _lib.device_guard(el.device):
        plan_r = get_plan(row, indptr_r, eid_r, indices_r, er.size(0))
        plan_c = get_plan(col, indptr_c, eid_c, indices_c, el.size(0))
        check(lib().graphop_gat_scores_backward(
            dtype_code(el), ptr(row), ptr(indptr_r), ptr(eid_r), ptr(indices_r), ptr(col), ptr(indptr_c),
            ptr(eid_c), ptr(indices_c), ptr(el), ptr(er), ptr(dy), ptr(d_el), ptr(d_er), row.size(0), col.size(0),
            e, el.size(0), er.size(0), h, float(negative_slope), plan_r.handle, plan_c.handle, stream_of(el)))
    return [d_el, d_er]


# ---- GATv2 attention scores (extra op) -----------------------------------------------------------------------------
def _gatv2_shapes(xl, xr, att, fn):
    """(h, d) of the GATv2 operands: xl (n_src, d), xr (n_dst, d), att (d) for one head, else (n, h, d) and (h, d)."""
    _same_dtype(xl, xr, "xl", "xr")
    _same_dtype(xl, att, "xl", "att")
    if xl.dim() not in (2, 3) or xr.dim() != xl.dim() or (xl.dim() == 3 and xl.size(1) != xr.size(1)):
        raise RuntimeError("%s: xl (n_src[, h], d) and xr (n_dst[, h], d) must have the same h, got %s and %s"
                           % (fn, tuple(xl.shape), tuple(xr.shape)))
    if xl.size(-1) != xr.size(-1):
        raise RuntimeError("%s: xl and xr must have the same d, got %s and %s" % (fn, tuple(xl.shape), tuple(xr.shape)))
    if tuple(att.shape) != tuple(xl.shape[1:]):
        raise RuntimeError("%s: att must be %s (the same h and the same d as xl), got %s"
                           % (fn, tuple(xl.shape[1:]), tuple(att.shape)))
    return (1 if xl.dim() == 2 else xl.size(1)), xl.size(-1)


def _gatv2_workspace_values(n_row_chunks, h, d):
    """the workspace minimum of graphop_gatv2_scores_backward (include/graphop_hip.h), in values"""
    return min((n_row_chunks + 15) // 16, 8192) * h * d


def gatv2_scores_forward(row, indptr, eid, indices, xl, xr, att, negative_slope=0.2):
    """y[eid[j], k] = sum_c att[k, c] * LeakyReLU(xl[row[c], k, c] + xr[indices[j], k, c], negative_slope);
    xl (n_src, d), xr (n_dst, d), att (d) give y (e); xl (n_src, h, d), xr (n_dst, h, d), att (h, d) give y (e, h)"""
    _check_csr((row, indptr, eid, indices), _CSR, (xl, "xl"), (xr, "xr"), (att, "att"))
    h, d = _gatv2_shapes(xl, xr, att, "gatv2_scores_forward")
    e = eid.size(0)
    y = torch.empty((e,) if xl.dim() == 2 else (e, h), dtype=xl.dtype, device=xl.device)
    with _lib.device_guard(xl.device):
        plan = get_plan(row, indptr, eid, indices, xr.size(0))
        check(lib().graphop_gatv2_scores_forward(
            dtype_code(xl), ptr(row), ptr(indptr), ptr(eid), ptr(indices), ptr(xl), ptr(xr), ptr(att), ptr(y),
            row.size(0), e, xl.size(0), xr.size(0), h, d, float(negative_slope), plan.handle, stream_of(xl)))
    return y


def gatv2_scores_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, att, dy,
                          negative_slope=0.2):
    """-> [dxl, dxr, datt] of gatv2_scores_forward for the score gradient dy (z is recomputed from xl and xr)"""
    _check_csr((row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c), _CSR_RC,
               (xl, "xl"), (xr, "xr"), (att, "att"))
    _check_grad(dy, "dy")
    h, d = _gatv2_shapes(xl, xr, att, "gatv2_scores_backward")
    _same_dtype(xl, dy, "xl", "dy")
    dy = dy.contiguous()
    e = eid_r.size(0)
    if dy.numel() != e * h:
        raise RuntimeError("gatv2_scores_backward: dy must hold (n_edges, h) = (%d, %d) values, got %s"
                           % (e, h, tuple(dy.shape)))
    dxl, dxr, datt = torch.empty_like(xl), torch.empty_like(xr), torch.empty_like(att)
    ws = torch.empty(max(_gatv2_workspace_values(row.size(0), h, d), 1), dtype=xl.dtype, device=xl.device)
    with _lib.device_guard(xl.device):
        plan_r = get_plan(row, indptr_r, eid_r, indices_r, xr.size(0))
        plan_c = get_plan(col, indptr_c, eid_c, indices_c, xl.size(0))
        check(lib().graphop_gatv2_scores_backward(
            dtype_code(xl), ptr(row), ptr(indptr_r), ptr(eid_r), ptr(indices_r), ptr(col), ptr(indptr_c),
            ptr(eid_c), ptr(indices_c), ptr(xl), ptr(xr), ptr(att), ptr(dy), ptr(dxl), ptr(dxr), ptr(datt), ptr(ws),
            ws.numel() * ws.element_size(), row.size(0), col.size(0), e, xl.size(0), xr.size(0), h, d,
            float(negative_slope), plan_r.handle, plan_c.handle, stream_of(xl)))
    return [dxl, dxr, datt]


# ---- the fused layers (extra ops) ---------------------------------------------------------------------------------
def _saved_checked(fn, oshape, n_src, h, o, stats, dO):
    """What a fused backward saved from its forward, o (oshape) and stats (n_src, h, 2), and the gradient of o, checked
    against each other -> that gradient, contiguous."""
    if o.shape != oshape or stats.numel() != n_src * h * 2:
        raise RuntimeError("%s: o must be %s and stats (n_src, h, 2), got %s and %s"
                           % (fn, oshape, tuple(o.shape), tuple(stats.shape)))
    dO = dO.contiguous()
    if dO.shape != o.shape:
        raise RuntimeError("%s: dO must match o %s, got %s" % (fn, tuple(o.shape), tuple(dO.shape)))
    return dO


# ---- fused GATv2 attention (extra op) ---------------------------------------------------------------------------
def _gatv2_attention_workspace_values(n_l, n_row_chunks, h, d):
    """the workspace minimum of graphop_gatv2_attention_backward (include/graphop_hip.h), in values"""
    return n_l * h * 4 + min((n_row_chunks + 15) // 16, 8192) * h * d


def _gatv2_edge_rows(xl, xe, n_edges, h, d, fn):
    """xe checked against the graph and xl: (n_edges, d) for 2-D xl / xr, else (n_edges, h, d), in xl's dtype."""
    _check_input(xe, "xe")
    _same_dtype(xl, xe, "xl", "xe")
    want = (n_edges, d) if xl.dim() == 2 else (n_edges, h, d)
    if xe.dim() == len(want) and tuple(xe.shape[1:]) == want[1:]:
        _check_edge_rows(xe, "xe", n_edges)
    if tuple(xe.shape) != want:
        raise RuntimeError("%s: xe must be (n_edges, d) for 2-D xl / xr, else (n_edges, h, d) with n_edges = %d, h = %d "
                           "and d = %d, got xe %s, xl %s" % (fn, n_edges, h, d, tuple(xe.shape), tuple(xl.shape)))


def _gatv2_attention_forward(fn, row, indptr, eid, indices, xl, xr, att, negative_slope, drop=(), xe=None):
    """gatv2_attention_forward (drop = ()) or gatv2_attention_dropout_forward (drop = (p, seed, offset)) as `fn`; with the
    edge rows xe (which need drop) the C entry point is graphop_gatv2_edge_attention_forward."""
    edge = () if xe is None else (xe,)
    _check_csr((row, indptr, eid, indices), _CSR, (xl, "xl"), (xr, "xr"), (att, "att"))
    h, d = _gatv2_shapes(xl, xr, att, fn)
    e, n_l = eid.size(0), xl.size(0)
    if edge:
        _gatv2_edge_rows(xl, xe, e, h, d, fn)         # checks xe as an input too
    o = torch.empty_like(xl)
    stats = torch.empty((n_l, h, 2), dtype=xl.dtype, device=xl.device)
    with _lib.device_guard(xl.device):
        plan = get_plan(row, indptr, eid, indices, xr.size(0))
        check(getattr(lib(), "graphop_gatv2_edge_attention_forward" if edge else "graphop_" + fn)(
            dtype_code(xl), ptr(row), ptr(indptr), ptr(eid), ptr(indices), ptr(xl), ptr(xr), *(ptr(t) for t in edge),
            ptr(att), ptr(o), ptr(stats), row.size(0), e, n_l, xr.size(0), h, d, float(negative_slope), *drop,
            plan.handle, stream_of(xl)))
    return [o, stats]


def _gatv2_attention_backward(fn, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, att, o,
                              stats, dO, negative_slope, drop=(), xe=None, need_dxe=True):
    """gatv2_attention_backward (drop = ()) or gatv2_attention_dropout_backward (drop = (p, seed, offset)) as `fn`:
    -> [dxl, dxr, datt]; with the edge rows xe (which need drop) the C entry point is
    graphop_gatv2_edge_attention_backward: -> [dxl, dxr, datt, dxe]."""
    edge = () if xe is None else (xe,)
    _check_csr((row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c), _CSR_RC,
               (xl, "xl"), (xr, "xr"), (att, "att"), (o, "o"), (stats, "stats"))
    _check_grad(dO, "dO")
    h, d = _gatv2_shapes(xl, xr, att, fn)
    e, n_l = eid_r.size(0), xl.size(0)
    if edge:
        _gatv2_edge_rows(xl, xe, e, h, d, fn)         # checks xe as an input too
    for t, n in ((o, "o"), (stats, "stats"), (dO, "dO")):
        _same_dtype(xl, t, "xl", n)
    dO = _saved_checked(fn, tuple(xl.shape), n_l, h, o, stats, dO)
    dxl, dxr, datt = torch.empty_like(xl), torch.empty_like(xr), torch.empty_like(att)
    dxe = ()        # with xe: [dxe], an empty (0,) tensor and a NULL pointer where it is not wanted
    if edge:
        dxe = (torch.empty_like(xe) if need_dxe else torch.empty((0,), dtype=xe.dtype, device=xe.device),)
    ws = torch.empty(max(_gatv2_attention_workspace_values(n_l, row.size(0), h, d), 1), dtype=xl.dtype,
                     device=xl.device)
    with _lib.device_guard(xl.device):
        plan_r = get_plan(row, indptr_r, eid_r, indices_r, xr.size(0))
        plan_c = get_plan(col, indptr_c, eid_c, indices_c, n_l)
        check(getattr(lib(), "graphop_gatv2_edge_attention_backward" if edge else "graphop_" + fn)(
            dtype_code(xl), ptr(row), ptr(indptr_r), ptr(eid_r), ptr(indices_r), ptr(col), ptr(indptr_c),
            ptr(eid_c), ptr(indices_c), ptr(xl), ptr(xr), *(ptr(t) for t in edge), ptr(att), ptr(o), ptr(stats),
            ptr(dO), ptr(dxl), ptr(dxr), *(ptr(t) if need_dxe else _NULL for t in dxe), ptr(datt), ptr(ws),
            ws.numel() * ws.element_size(), row.size(0), col.size(0), e, n_l, xr.size(0), h, d,
            float(negative_slope), *drop, plan_r.handle, plan_c.handle, stream_of(xl)))
    return [dxl, dxr, datt, *dxe]


def gatv2_attention_forward(row, indptr, eid, indices, xl, xr, att, negative_slope=0.2):
    """-> [o, stats]: o[i] = sum_j softmax_j(att . LeakyReLU(xl[i] + xr[j])) xr[j] per head over the row-major CSR,
    without any E-sized tensor; o has n_src = xl.size(0) rows in xl's layout, stats (n_src, h, 2) = (row max, 1 / sum exp)."""
    return _gatv2_attention_forward("gatv2_attention_forward", row, indptr, eid, indices, xl, xr, att, negative_slope)


def gatv2_attention_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, att, o, stats,
                             dO, negative_slope=0.2):
    """-> [dxl, dxr, datt] of gatv2_attention_forward for the output gradient dO (z, s and a recomputed per slot from
    xl, xr, att and stats)."""
    return _gatv2_attention_backward("gatv2_attention_backward", row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c,
                                     indices_c, xl, xr, att, o, stats, dO, negative_slope)


# ---- fused GAT attention (extra op) -----------------------------------------------------------------------------
def _gat_attn_shapes(el, er, V, fn):
    """(h, d) of the fused GAT layer: V is (n_dst, d) with 1-D el / er, else (n_dst, h, d), in their dtype."""
    h = _gat_heads(el, er, fn)
    _same_dtype(el, V, "el", "V")
    if V.dim() != (2 if el.dim() == 1 else 3) or (V.dim() == 3 and V.size(1) != h) or V.size(0) != er.size(0):
        raise RuntimeError("%s: V must be (n_dst, d) for 1-D el / er, else (n_dst, h, d) with the same h and n_dst as er, "
                           "got V %s, er %s" % (fn, tuple(V.shape), tuple(er.shape)))
    return h, V.size(-1)


def _gat_attention_forward(fn, row, indptr, eid, indices, el, er, V, negative_slope, drop=(), ee=None):
    """gat_attention_forward (drop = ()), gat_attention_dropout_forward or, with the edge term ee,
    gat_edge_attention_forward (drop = (p, seed, offset)) as `fn`."""
    edge = () if ee is None else (ee,)
    _check_csr((row, indptr, eid, indices), _CSR, (el, "el"), (er, "er"), (V, "V"))
    h, d = _gat_attn_shapes(el, er, V, fn)
    e, n_l = eid.size(0), el.size(0)
    if edge:
        _gat_edge_term(el, ee, e, h, fn)         # checks ee as an input too
    o = torch.empty((n_l,) + tuple(V.shape[1:]), dtype=V.dtype, device=V.device)
    stats = torch.empty((n_l, h, 2), dtype=el.dtype, device=el.device)
    with _lib.device_guard(el.device):
        plan = get_plan(row, indptr, eid, indices, er.size(0))
        check(getattr(lib(), "graphop_" + fn)(
            dtype_code(el), ptr(row), ptr(indptr), ptr(eid), ptr(indices), ptr(el), ptr(er), *(ptr(t) for t in edge),
            ptr(V), ptr(o), ptr(stats), row.size(0), e, n_l, er.size(0), h, d, float(negative_slope), *drop,
            plan.handle, stream_of(el)))
    return [o, stats]


def _gat_attention_backward(fn, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, V, o, stats,
                            dO, negative_slope, drop=(), ee=None, need_dee=True):
    """gat_attention_backward (drop = ()), gat_attention_dropout_backward or, with the edge term ee,
    gat_edge_attention_backward (drop = (p, seed, offset)) as `fn`: -> [del, der, dV], with ee [del, der, dee, dV]."""
    edge = () if ee is None else (ee,)
    _check_csr((row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c), _CSR_RC,
               (el, "el"), (er, "er"), (V, "V"), (o, "o"), (stats, "stats"))
    _check_grad(dO, "dO")
    h, d = _gat_attn_shapes(el, er, V, fn)
    e, n_l = eid_r.size(0), el.size(0)
    if edge:
        _gat_edge_term(el, ee, e, h, fn)         # checks ee as an input too
    for t, n in ((o, "o"), (stats, "stats"), (dO, "dO")):
        _same_dtype(el, t, "el", n)
    dO = _saved_checked(fn, (n_l,) + tuple(V.shape[1:]), n_l, h, o, stats, dO)
    d_el, d_er, dV = torch.empty_like(el), torch.empty_like(er), torch.empty_like(V)
    d_ee = ()       # with ee: [dee], an empty (0,) tensor and a NULL pointer where it is not wanted
    if edge:
        d_ee = (torch.empty_like(ee) if need_dee else torch.empty((0,), dtype=ee.dtype, device=ee.device),)
    ws = torch.empty(max(n_l * h * 4, 1), dtype=el.dtype, device=el.device)      # (el, m, 1 / l, D) per (node, head)
    with _lib.device_guard(el.device):
        plan_r = get_plan(row, indptr_r, eid_r, indices_r, er.size(0))
        plan_c = get_plan(col, indptr_c, eid_c, indices_c, n_l)
        check(getattr(lib(), "graphop_" + fn)(
            dtype_code(el), ptr(row), ptr(indptr_r), ptr(eid_r), ptr(indices_r), ptr(col), ptr(indptr_c),
            ptr(eid_c), ptr(indices_c), ptr(el), ptr(er), *(ptr(t) for t in edge), ptr(V), ptr(o), ptr(stats),
            ptr(dO), ptr(d_el), ptr(d_er), *(ptr(t) if need_dee else _NULL for t in d_ee), ptr(dV), ptr(ws),
            ws.numel() * ws.element_size(), row.size(0), col.size(0), e, n_l, er.size(0), h, d,
            float(negative_slope), *drop, plan_r.handle, plan_c.handle, stream_of(el)))
    return [d_el, d_er, *d_ee, dV]


def gat_attention_forward(row, indptr, eid, indices, el, er, V, negative_slope=0.2):
    """-> [o, stats]: o[i] = sum_j softmax_j(LeakyReLU(el[i] + er[j])) V[j] per head over the row-major CSR, without
    any E-sized tensor; o has n_src = el.size(0) rows in V's layout, stats (n_src, h, 2) = (row max, 1 / sum exp)."""
    return _gat_attention_forward("gat_attention_forward", row, indptr, eid, indices, el, er, V, negative_slope)


def gat_attention_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, V, o, stats,
                           dO, negative_slope=0.2):
    """-> [del, der, dV] of gat_attention_forward for the output gradient dO (a recomputed per slot from stats)."""
    return _gat_attention_backward("gat_attention_backward", row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c,
                                   indices_c, el, er, V, o, stats, dO, negative_slope)


# ---- attention dropout of the fused GAT layer (extra ops) ------------------------------------------------------
def _drop_args(fn, p, seed, offset):
    """(p, seed, offset) checked as the C ABI states them: 0 <= p < 1, 0 <= seed < 2^63, 0 <= offset < 2^32."""
    p, seed, offset = float(p), int(seed), int(offset)
    if not 0.0 <= p < 1.0:
        raise RuntimeError("%s: dropout probability p must be in [0, 1), got %r" % (fn, p))
    if not 0 <= seed < 2 ** 63:
        raise RuntimeError("%s: seed must be in [0, 2^63), got %d" % (fn, seed))
    if not 0 <= offset < 2 ** 32:
        raise RuntimeError("%s: offset must be in [0, 2^32), got %d" % (fn, offset))
    return p, seed, offset


def gat_attention_dropout_forward(row, indptr, eid, indices, el, er, V, negative_slope=0.2, p=0.0, seed=0, offset=0):
    """-> [o, stats] of gat_attention_forward with dropout on the attention weights: o[i] = sum_j a_ij m_ij V[j],
    m_ij = keep(i, j, head; seed, offset, p) / (1 - p) recomputed per slot from Philox4x32-10 (no edge-sized mask);
    stats are those of the undropped scores.  p = 0 is gat_attention_forward bit for bit."""
    fn = "gat_attention_dropout_forward"
    return _gat_attention_forward(fn, row, indptr, eid, indices, el, er, V, negative_slope,
                                  _drop_args(fn, p, seed, offset))


def gat_attention_dropout_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, V, o,
                                   stats, dO, negative_slope=0.2, p=0.0, seed=0, offset=0):
    """-> [del, der, dV] of gat_attention_dropout_forward for the output gradient dO, with the same (p, seed, offset):
    the weights and their keep decisions are recomputed per slot."""
    fn = "gat_attention_dropout_backward"
    return _gat_attention_backward(fn, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, V, o,
                                   stats, dO, negative_slope, _drop_args(fn, p, seed, offset))


def gatv2_attention_dropout_forward(row, indptr, eid, indices, xl, xr, att, negative_slope=0.2, p=0.0, seed=0,
                                    offset=0, xe=None):
    """-> [o, stats] of gatv2_attention_forward with dropout on the attention weights: o[i] = sum_j a_ij m_ij xr[j], m_ij
    the multiplier of gat_attention_dropout_forward (i indexes xl, j indexes xr; no edge-sized mask); stats are those of
    the undropped scores, bit for bit.  p = 0 is gatv2_attention_forward bit for bit.
    xe: edge features (GATv2Conv(edge_dim=...)), indexed by edge id: (n_edges, d) for 2-D xl / xr, else (n_edges, h, d).
    For edge e = (i, j) the score is att . LeakyReLU((xl[i] + xr[j]) + xe[e]); xe is streamed once and nothing else
    edge-sized is made.  xe=None is the op without them, bit for bit."""
    fn = "gatv2_attention_dropout_forward"
    return _gatv2_attention_forward(fn, row, indptr, eid, indices, xl, xr, att, negative_slope,
                                    _drop_args(fn, p, seed, offset), xe)


def gatv2_attention_dropout_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, att, o,
                                     stats, dO, negative_slope=0.2, p=0.0, seed=0, offset=0, xe=None, need_dxe=True):
    """-> [dxl, dxr, datt] of gatv2_attention_dropout_forward for the output gradient dO, with the same (p, seed,
    offset): scores, weights and their keep decisions are recomputed per slot.
    With the edge features xe of the forward: -> [dxl, dxr, datt, dxe]; dxe[e] = ds att t in xe's shape is the only
    edge-sized tensor made (edge ids that no row-major slot names get 0); with need_dxe=False it is an empty (0,) tensor
    and nothing edge-sized is written."""
    fn = "gatv2_attention_dropout_backward"
    return _gatv2_attention_backward(fn, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, att,
                                     o, stats, dO, negative_slope, _drop_args(fn, p, seed, offset), xe, need_dxe)


def edge_dropout_mask(row, indptr, eid, indices, h, p, seed, offset=0, dtype=torch.float32):
    """-> the multipliers m[e, k] = keep(i, j, k) / (1 - p) the dropout ops above apply, as an edge tensor: (E) for
    h == 1, else (E, h).  (row, indptr, eid, indices) is the ROW-MAJOR CSR (i = row[c], j = indices[slot])."""
    p, seed, offset = _drop_args("edge_dropout_mask", p, seed, offset)
    _check_csr((row, indptr, eid, indices), _CSR)
    h = int(h)
    if h < 1 or dtype not in (torch.float32, torch.float64):
        raise RuntimeError("edge_dropout_mask: h must be >= 1 and dtype float32 or float64, got h=%d dtype=%s"
                           % (h, dtype))
    e = eid.size(0)
    y = _edge_out(e, h, dtype, row.device)
    bound = 2 ** 32 - 1       # the ids themselves are the only bound on the two node counts
    with _lib.device_guard(row.device):
        plan = get_plan(row, indptr, eid, indices, 0)
        n_l = max(plan.info.max_row + 1, 0) if e else 0
        n_r = max(plan.info.max_index + 1, 0) if e else 0
        check(lib().graphop_edge_dropout_mask(
            dtype_code(y), ptr(row), ptr(indptr), ptr(eid), ptr(indices), ptr(y), row.size(0), e, min(n_l, bound),
            min(n_r, bound), h, p, seed, offset, plan.handle, stream_of(row)))
    return y


# ---- attention dropout of the fused attention step (extra ops) -----------------------------------------------------
def _head0(fn, head0):
    head0 = int(head0)
    if not 0 <= head0 < 2 ** 32:
        raise RuntimeError("%s: head0 must be in [0, 2^32), got %d" % (fn, head0))
    return head0


def attention_dropout_forward(row, indptr, eid, indices, Q, K, V, p=0.0, seed=0, offset=0, head0=0):
    """-> [o, stats] of attention_forward with dropout on the attention weights: o[i] = sum_j a_ij m_ij V[j], m_ij the
    multiplier of edge_dropout_mask (i indexes Q, j indexes K / V) recomputed per slot, so no edge-sized mask exists;
    stats are those of the undropped scores.  head0 is the global index of the call's first head: head k of this call
    decides as head head0 + k of edge_dropout_mask (the head groups of FusedAttentionDropout pass their first head).
    p = 0 is attention_forward bit for bit.  There is no 1 / sqrt(d) scale argument: fold it into Q."""
    fn = "attention_dropout_forward"
    return _attention_forward(fn, row, indptr, eid, indices, Q, K, V, _drop_args(fn, p, seed, offset) + (_head0(fn, head0),))


def attention_dropout_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, o, stats, dO,
                               p=0.0, seed=0, offset=0, head0=0):
    """-> [dQ, dK, dV] of attention_dropout_forward for the output gradient dO, with the same (p, seed, offset, head0):
    the weights and their keep decisions are recomputed per slot."""
    fn = "attention_dropout_backward"
    return _attention_backward(fn, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, o, stats,
                               dO, _drop_args(fn, p, seed, offset) + (_head0(fn, head0),))


# ---- per-edge score bias of the fused attention step (extra ops) ------------------------------------
def attention_bias_forward(row, indptr, eid, indices, Q, K, V, b, p=0.0, seed=0, offset=0, head0=0):
    """-> [o, stats] of attention_dropout_forward with a term per edge inside the softmax: for edge e = (i, j),
    s_e = <Q_i, K_j> + b[e], a = row-softmax(s), o[i] = sum_e a_e m_e V[j].  b is indexed by edge id ((n_edges) for 2-D
    Q / K / V, else (n_edges, h)), has their dtype and is contiguous: a Graphormer-type spatial / edge encoding, a
    relative positional bias, log w of a weighted graph, or node_mul_edge_forward(Q, xe) for the key-side edge term of
    TransformerConv(edge_dim=...) alone (that layer also adds the edge row to the value: attention_edge_forward has both
    terms).  b must be finite: a bias at or below the -1e9 floor of the row maximum is not a mask.
    stats are those of the biased, undropped scores; (p, seed, offset, head0) as attention_dropout_forward, p = 0: no
    dropout.  There is no 1 / sqrt(d) scale argument: fold it into Q."""
    fn = "attention_bias_forward"
    return _attention_forward(fn, row, indptr, eid, indices, Q, K, V,
                              _drop_args(fn, p, seed, offset) + (_head0(fn, head0),), b)


def attention_bias_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, b, o, stats, dO,
                            p=0.0, seed=0, offset=0, head0=0, need_db=True):
    """-> [dQ, dK, dV, db] of attention_bias_forward for the output gradient dO, with the same (p, seed, offset, head0):
    the weights and their keep decisions are recomputed per slot.  db[e] = ds_e in b's shape is the only edge-sized
    tensor made; with need_db=False it is an empty (0,) tensor and nothing edge-sized is written.  b must be finite (a
    bias at or below the -1e9 floor is not a mask)."""
    fn = "attention_bias_backward"
    return _attention_backward(fn, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, o, stats,
                               dO, _drop_args(fn, p, seed, offset) + (_head0(fn, head0),), b, need_db)


# ---- an edge row in key and value of the fused attention step (extra ops): K_j + xe[e], V_j + xe[e]
# ---- and, for a categorical edge feature, K_j + R[t_e], V_j + R[t_e] (4.5o) or <Q_i, K_j> + B[t_e] (4.5p).  One body
# ---- per direction: etype None is the first op (rows = xe), else the op's name says which table rows is (R or B)
def _attn_edge_rows(fn, xe, Q, n_edges):
    """xe checked against the graph and Q: a contiguous device tensor (n_edges, d) for 2-D Q / K / V, else
    (n_edges, h, d), in Q's dtype.  The C ABI takes a raw pointer: each of these would read out of bounds or garbage."""
    _same_dtype(Q, xe, "Q", "xe")
    if tuple(xe.shape) != (n_edges,) + tuple(Q.shape[1:]):
        raise RuntimeError("%s: xe must be (n_edges, d) for 2-D Q / K / V, else (n_edges, h, d) with n_edges = %d, "
                           "got xe %s, Q %s" % (fn, n_edges, tuple(xe.shape), tuple(Q.shape)))
    if not xe.is_contiguous():
        raise RuntimeError("xe must be contiguous")
    if not xe.is_cuda:
        raise RuntimeError("xe must be a CUDA tensor")


def _attn_etype_table(fn, R, etype, Q, n_edges):
    """R and etype checked against the graph and Q: R a contiguous device tensor (n_types, d) for 2-D Q / K / V, else
    (n_types, h, d), in Q's dtype, with n_types >= 1 unless the graph has no edge; etype a contiguous device int32
    tensor (n_edges).  The C ABI takes raw pointers: each of these would read out of bounds or garbage.  The VALUES of
    etype are not looked at (that would synchronise): the kernels clamp them."""
    _same_dtype(Q, R, "Q", "R")
    if R.dim() != Q.dim() or tuple(R.shape[1:]) != tuple(Q.shape[1:]):
        raise RuntimeError("%s: R must be (n_types, d) for 2-D Q / K / V, else (n_types, h, d), got R %s, Q %s"
                           % (fn, tuple(R.shape), tuple(Q.shape)))
    if R.size(0) == 0 and n_edges > 0:
        raise RuntimeError("%s: R must hold at least one type (n_edges = %d)" % (fn, n_edges))
    if etype.dtype != torch.int32:
        raise RuntimeError("%s: etype must be torch.int32, got %s" % (fn, etype.dtype))
    if tuple(etype.shape) != (n_edges,):
        raise RuntimeError("%s: etype must be (n_edges) with n_edges = %d, got %s" % (fn, n_edges, tuple(etype.shape)))
    for t, n in ((R, "R"), (etype, "etype")):
        if not t.is_contiguous():
            raise RuntimeError("%s must be contiguous" % n)
        if not t.is_cuda:
            raise RuntimeError("%s must be a CUDA tensor" % n)


def _attn_tbias_table(fn, B, etype, Q, n_edges):
    """B and etype checked against the graph and Q: B a contiguous device tensor (n_types) for 2-D Q / K / V, else
    (n_types, h), in Q's dtype, with n_types >= 1 unless the graph has no edge; etype a contiguous device int32 tensor
    (n_edges).  The C ABI takes raw pointers: each of these would read out of bounds or garbage.  The VALUES of etype
    are not looked at (that would synchronise): the kernels clamp them."""
    _same_dtype(Q, B, "Q", "B")
    if B.dim() != Q.dim() - 1 or tuple(B.shape[1:]) != tuple(Q.shape[1:-1]):
        raise RuntimeError("%s: B must be (n_types) for 2-D Q / K / V, else (n_types, h), got B %s, Q %s"
                           % (fn, tuple(B.shape), tuple(Q.shape)))
    if B.size(0) == 0 and n_edges > 0:
        raise RuntimeError("%s: B must hold at least one type (n_edges = %d)" % (fn, n_edges))
    if etype.dtype != torch.int32:
        raise RuntimeError("%s: etype must be torch.int32, got %s" % (fn, etype.dtype))
    if tuple(etype.shape) != (n_edges,):
        raise RuntimeError("%s: etype must be (n_edges) with n_edges = %d, got %s" % (fn, n_edges, tuple(etype.shape)))
    for t, n in ((B, "B"), (etype, "etype")):
        if not t.is_contiguous():
            raise RuntimeError("%s must be contiguous" % n)
        if not t.is_cuda:
            raise RuntimeError("%s must be a CUDA tensor" % n)


def _attn_edge_form(fn):
    """"edge", "etype" or "tbias": the form an op's name attention_<form>_<direction> carries"""
    return fn.split("_")[1]


def _attn_edge_workspace(like, backward, sizes, plan_r, plan_c, form):
    """sizes: (e, n_q, n_k, h, d) and, with a table, n_types"""
    import ctypes
    nbytes = ctypes.c_int64(0)
    query = getattr(lib(), "graphop_attention_%s_workspace_bytes" % form)
    check(query(dtype_code(like), 1 if backward else 0, *sizes, plan_r.handle,
                plan_c.handle if plan_c is not None else _NULL, stream_of(like), ctypes.byref(nbytes)))
    return torch.empty(max(1, nbytes.value), dtype=torch.uint8, device=like.device), nbytes.value


def _attn_edge_operands(fn, rows, etype, Q, e, n_q, n_k, h, d):
    """the form's operand check -> (its pointer arguments, the size arguments of its calls)"""
    if etype is None:
        _attn_edge_rows(fn, rows, Q, e)
        return (ptr(rows),), (e, n_q, n_k, h, d)
    (_attn_tbias_table if _attn_edge_form(fn) == "tbias" else _attn_etype_table)(fn, rows, etype, Q, e)
    return (ptr(rows), ptr(etype)), (e, n_q, n_k, h, d, rows.size(0))


def _attn_edge_forward(fn, row, indptr, eid, indices, Q, K, V, rows, etype, p, seed, offset, head0):
    drop = _drop_args(fn, p, seed, offset) + (_head0(fn, head0),)
    _check_csr((row, indptr, eid, indices), _CSR, (Q, "Q"), (K, "K"), (V, "V"))
    _same_dtype(Q, K, "Q", "K")
    _same_dtype(Q, V, "Q", "V")
    if K.shape != V.shape or Q.shape[1:] != K.shape[1:]:
        raise RuntimeError("%s: Q (n_q,[h,]d), K and V (n_k,[h,]d) expected" % fn)
    e, d = eid.size(0), Q.size(-1)
    h = 1 if Q.dim() == 2 else Q.size(1)
    n_q, n_k = Q.size(0), K.size(0)
    form = _attn_edge_form(fn)
    operands, sizes = _attn_edge_operands(fn, rows, etype, Q, e, n_q, n_k, h, d)
    o = torch.empty_like(Q)
    stats = torch.empty((n_q, h, 2), dtype=Q.dtype, device=Q.device)
    with _lib.device_guard(Q.device):
        plan = get_plan(row, indptr, eid, indices, n_k)
        ws, nbytes = _attn_edge_workspace(Q, False, sizes, plan, None, form)
        call = getattr(lib(), "graphop_" + fn)
        check(call(dtype_code(Q), ptr(row), ptr(indptr), ptr(eid), ptr(indices), ptr(Q), ptr(K), ptr(V), *operands,
                   ptr(o), ptr(stats), row.size(0), *sizes, ptr(ws), nbytes, plan.handle, stream_of(Q), *drop))
    return [o, stats]


def _attn_edge_backward(fn, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, rows, etype, o,
                        stats, dO, p, seed, offset, head0, need_dx):
    drop = _drop_args(fn, p, seed, offset) + (_head0(fn, head0),)
    _check_csr((row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c), _CSR_RC,
               (Q, "Q"), (K, "K"), (V, "V"), (o, "o"), (stats, "stats"))
    _check_grad(dO, "dO")
    for t, n in ((K, "K"), (V, "V"), (o, "o"), (stats, "stats"), (dO, "dO")):
        _same_dtype(Q, t, "Q", n)
    dO = dO.contiguous()
    if K.shape != V.shape or Q.shape[1:] != K.shape[1:]:
        raise RuntimeError("%s: Q (n_q,[h,]d), K and V (n_k,[h,]d) expected" % fn)
    e, d = eid_r.size(0), Q.size(-1)
    h = 1 if Q.dim() == 2 else Q.size(1)
    n_q, n_k = Q.size(0), K.size(0)
    if o.shape != Q.shape or dO.shape != Q.shape or stats.numel() != n_q * h * 2:
        raise RuntimeError("%s: o, dO must match Q and stats must be (n_q, h, 2)" % fn)
    form = _attn_edge_form(fn)
    operands, sizes = _attn_edge_operands(fn, rows, etype, Q, e, n_q, n_k, h, d)
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    with _lib.device_guard(Q.device):
        plan_r = get_plan(row, indptr_r, eid_r, indices_r, n_k)
        plan_c = get_plan(col, indptr_c, eid_c, indices_c, n_q)
        # dR, dB: the call fills it.  dxe[e] is written once per row-major slot: only a chunk list that leaves slots out
        # needs the zeros
        if not need_dx:
            dx = torch.empty((0,), dtype=rows.dtype, device=rows.device)
        else:
            dx = torch.empty_like(rows) if form != "edge" or plan_r.info.full_coverage else torch.zeros_like(rows)
        ws, nbytes = _attn_edge_workspace(Q, True, sizes, plan_r, plan_c, form)
        call = getattr(lib(), "graphop_" + fn)
        check(call(dtype_code(Q), ptr(row), ptr(indptr_r), ptr(eid_r), ptr(indices_r), ptr(col), ptr(indptr_c),
                   ptr(eid_c), ptr(indices_c), ptr(Q), ptr(K), ptr(V), *operands, ptr(o), ptr(stats), ptr(dO), ptr(dQ),
                   ptr(dK), ptr(dV), ptr(dx) if need_dx else _NULL, row.size(0), col.size(0), *sizes, ptr(ws), nbytes,
                   plan_r.handle, plan_c.handle, stream_of(Q), *drop))
    return [dQ, dK, dV, dx]


def attention_edge_forward(row, indptr, eid, indices, Q, K, V, xe, p=0.0, seed=0, offset=0, head0=0):
    """-> [o, stats] of the fused attention step with a feature row per edge added to the key AND the value: for edge
    e = (i, j),  kx = K[j] + xe[e],  vx = V[j] + xe[e],  s_e = <Q_i, kx_e>,  a = row-softmax(s),  o[i] = sum_e a_e m_e vx_e
    (TransformerConv(edge_dim=...): out = alpha * (value_j + edge_attr); the Dwivedi-Bresson and GraphGPS edge-featured
    graph transformers).  xe is indexed by edge id ((n_edges, d) for 2-D Q / K / V, else (n_edges, h, d)), has their
    dtype and is contiguous; parallel edges share a dropout decision and have each their own row.  stats (n_q, h, 2) =
    (row max floored at -1e9, 1 / sum exp) of the undropped scores, (-1e9, 0) and o = 0 for rows without edges;
    (p, seed, offset, head0) as attention_dropout_forward, p = 0: no dropout.  Nothing edge-sized is made.  There is no
    1 / sqrt(d) scale argument (fold it into Q) and no bias argument."""
    return _attn_edge_forward("attention_edge_forward", row, indptr, eid, indices, Q, K, V, xe, None, p, seed, offset, head0)


def attention_edge_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, xe, o, stats, dO,
                            p=0.0, seed=0, offset=0, head0=0, need_dxe=True):
    """-> [dQ, dK, dV, dxe] of attention_edge_forward for the output gradient dO, with the same (p, seed, offset,
    head0): the weights and their keep decisions are recomputed per slot.  dxe[e] = ds_e Q_i + a_e m_e dO_i in xe's
    shape is the only edge-sized tensor made (edge ids that no row-major slot names get 0); with need_dxe=False it is
    an empty (0,) tensor and nothing edge-sized is written."""
    return _attn_edge_backward("attention_edge_backward", row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c,
                               Q, K, V, xe, None, o, stats, dO, p, seed, offset, head0, need_dxe)


def attention_etype_forward(row, indptr, eid, indices, Q, K, V, R, etype, p=0.0, seed=0, offset=0, head0=0):
    """-> [o, stats] of attention_edge_forward for a categorical edge feature: edge e = (i, j) carries the type
    t = etype[e] and the table row R[t] is added to its key AND its value,  kx = K[j] + R[t],  vx = V[j] + R[t],
    s_e = <Q_i, kx_e>,  a = row-softmax(s),  o[i] = sum_e a_e m_e vx_e  (relation-aware attention, Shaw-type relative
    positions, TransformerConv(edge_dim=...) behind an nn.Embedding).  etype is (n_edges) torch.int32, contiguous,
    indexed by edge id, with values in [0, n_types); R is (n_types, d) for 2-D Q / K / V, else (n_types, h, d), in their
    dtype and contiguous.  Nothing of size (n_edges, h, d) is made or read: this is attention_edge_forward on
    R[etype.long()] without that tensor.  Parallel edges share a dropout decision and may differ in type.
    Out-of-range types: etype is not scanned (a scan would synchronise the stream and break its capture); every kernel
    clamps a type into [0, n_types - 1] before it forms an address, so a type outside [0, n_types) gives an undefined
    value and never touches memory outside R.  stats, (p, seed, offset, head0), the missing 1 / sqrt(d) and bias
    arguments: as attention_edge_forward."""
    return _attn_edge_forward("attention_etype_forward", row, indptr, eid, indices, Q, K, V, R, etype, p, seed, offset,
                              head0)


def attention_etype_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, R, etype, o,
                             stats, dO, p=0.0, seed=0, offset=0, head0=0, need_dR=True):
    """-> [dQ, dK, dV, dR] of attention_etype_forward for the output gradient dO, with the same (p, seed, offset,
    head0): the weights and their keep decisions are recomputed per slot.  dR[t] = sum over the edges of type t of
    (ds_e Q_i + a_e m_e dO_i) in R's shape is summed on chip -- no (n_edges, h, d) gradient exists -- and is 0 for a type
    no edge carries; with need_dR=False it is an empty (0,) tensor and nothing is accumulated.  Out-of-range types are
    clamped as in the forward: they never touch memory outside R / dR."""
    return _attn_edge_backward("attention_etype_backward", row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c,
                               indices_c, Q, K, V, R, etype, o, stats, dO, p, seed, offset, head0, need_dR)


def attention_tbias_forward(row, indptr, eid, indices, Q, K, V, B, etype, p=0.0, seed=0, offset=0, head0=0):
    """-> [o, stats] of attention_bias_forward for a categorical edge feature whose learned term is a scalar per
    (category, head) inside the softmax: edge e = (i, j) carries the type t = etype[e] and
    s_e = <Q_i, K_j> + B[t, k],  a = row-softmax(s),  o[i] = sum_e a_e m_e V[j]  (Graphormer's spatial encoding
    b_phi(i, j) and its edge encoding on bond types, T5 / Swin-type bucketed relative-position biases, relation biases of
    heterogeneous graphs).  etype is (n_edges) torch.int32, contiguous, indexed by edge id, with values in [0, n_types);
    B is (n_types) for 2-D Q / K / V, else (n_types, h), in their dtype, contiguous and finite.  Nothing of size
    (n_edges, h) is made or read: this is attention_bias_forward on B[etype.long()] without that tensor.  stats
    (n_q, h, 2) = (row max floored at -1e9, 1 / sum exp) of the biased, undropped scores -- attention_weights(...,
    b=B[etype.long()]) reproduces the weights from them -- and (-1e9, 0) with o = 0 for rows without edges.  Parallel
    edges share a dropout decision and may differ in type.
    Out-of-range types: etype is not scanned (a scan would synchronise the stream and break its capture); every kernel
    clamps a type into [0, n_types - 1] before it forms an address, so a type outside [0, n_types) gives an undefined
    value and never touches memory outside B.  (p, seed, offset, head0) as attention_dropout_forward, p = 0: no
    dropout.  There is no 1 / sqrt(d) scale argument (fold it into Q), and no per-edge b, xe or R together with B."""
    return _attn_edge_forward("attention_tbias_forward", row, indptr, eid, indices, Q, K, V, B, etype, p, seed, offset,
                              head0)


def attention_tbias_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, B, etype, o,
                             stats, dO, p=0.0, seed=0, offset=0, head0=0, need_dB=True):
    """-> [dQ, dK, dV, dB] of attention_tbias_forward for the output gradient dO, with the same (p, seed, offset,
    head0): the weights and their keep decisions are recomputed per slot.  dB[t] = sum over the edges of type t of ds_e
    in B's shape is summed on chip -- no (n_edges, h) gradient exists -- and is 0 for a type no edge carries; with
    need_dB=False it is an empty (0,) tensor and nothing is accumulated.  Out-of-range types are clamped as in the
    forward: they never touch memory outside B / dB."""
    return _attn_edge_backward("attention_tbias_backward", row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c,
                               indices_c, Q, K, V, B, etype, o, stats, dO, p, seed, offset, head0, need_dB)


# ---- the weights of the fused attention ops from their row statistics (extra op) ---------------------
def _attn_weights_operands(fn, Q, K, stats, b, xe, n_edges):
    """-> (h, d): the mode (at most one of b and xe), then Q, K and stats against each other, then b or xe against the
    graph and Q in the words of the ops that take them"""
    if b is not None and xe is not None:
        raise RuntimeError("%s: at most one of b and xe may be given" % fn)
    _same_dtype(Q, K, "Q", "K")
    _same_dtype(Q, stats, "Q", "stats")
    if Q.dim() not in (2, 3) or Q.shape[1:] != K.shape[1:]:
        raise RuntimeError("%s: Q (n_q,[h,]d) and K (n_k,[h,]d) expected" % fn)
    h = 1 if Q.dim() == 2 else Q.size(1)
    if tuple(stats.shape) != (Q.size(0), h, 2):
        raise RuntimeError("%s: stats must be (n_q, h, 2) = (%d, %d, 2), got %s"
                           % (fn, Q.size(0), h, tuple(stats.shape)))
    if b is not None:
        _attn_bias(fn, b, Q, n_edges, h)
    if xe is not None:
        _attn_edge_rows(fn, xe, Q, n_edges)
    return h, Q.size(-1)


def attention_weights(row, indptr, eid, indices, Q, K, stats, b=None, xe=None):
    """-> a, the attention weights of attention_forward / attention_dropout_forward (neither b nor xe),
    attention_bias_forward (b) or attention_edge_forward (xe) from the stats (n_q, h, 2) = (m_i, 1 / l_i) that op
    returned: for edge e = (i, j),  s_e = <Q_i, K_j> (+ b[e]) or <Q_i, K_j + xe[e]>,  a_e = exp(min(s_e - m_i, 0)) / l_i.
    a is indexed by edge id, (n_edges) for 2-D Q / K, else (n_edges, h): the layout of sparse_softmax_forward's result
    (PyG's return_attention_weights=True, DGL's get_attention=True).  These are the UNDROPPED weights; the effective
    ones are a * edge_dropout_mask(...).  The clamp keeps a <= 1 whichever forward produced the statistics.  Edge ids
    that no slot names read 0; giving b and xe together is an error.  One SDDMM plus one stream pass over a (plain,
    bias) or one gather pass (xe): no second softmax, no workspace, nothing of size (n_edges, h, d)."""
    fn = "attention_weights"
    _check_csr((row, indptr, eid, indices), _CSR, (Q, "Q"), (K, "K"), (stats, "stats"),
               *(((b, "b"),) if b is not None else ()))
    e, n_q, n_k = eid.size(0), Q.size(0), K.size(0)
    h, d = _attn_weights_operands(fn, Q, K, stats, b, xe, e)
    with _lib.device_guard(Q.device):
        plan = get_plan(row, indptr, eid, indices, n_k)
        # a[e] is written once per row-major slot: only a chunk list that leaves slots out needs the zeros
        shape = (e,) if Q.dim() == 2 else (e, h)
        a = (torch.empty if plan.info.full_coverage else torch.zeros)(shape, dtype=Q.dtype, device=Q.device)
        check(lib().graphop_attention_weights(
            dtype_code(Q), ptr(row), ptr(indptr), ptr(eid), ptr(indices), ptr(Q), ptr(K), ptr(stats),
            ptr(b) if b is not None else _NULL, ptr(xe) if xe is not None else _NULL, ptr(a), row.size(0), e, n_q, n_k,
            h, d, plan.handle, stream_of(Q)))
    return a


# ---- fused GAT attention with an edge term (extra ops) -----------------------------------------------------------
def _gat_edge_term(el, ee, n_edges, h, fn):
    """ee checked against the graph and the heads: (n_edges) for 1-D el / er, else (n_edges, h), in el's dtype."""
    _check_input(ee, "ee")
    _same_dtype(el, ee, "el", "ee")
    if tuple(ee.shape) != ((n_edges,) if el.dim() == 1 else (n_edges, h)):
        raise RuntimeError("%s: ee must be (n_edges) for 1-D el / er, else (n_edges, h) with n_edges = %d and h = %d, "
                           "got ee %s, el %s" % (fn, n_edges, h, tuple(ee.shape), tuple(el.shape)))


def gat_edge_attention_forward(row, indptr, eid, indices, el, er, ee, V, negative_slope=0.2, p=0.0, seed=0, offset=0):
    """-> [o, stats] of the fused GAT layer with a per-edge score term: for edge e = (i, j),
    s = LeakyReLU((el[i] + er[j]) + ee[e]), a = row-softmax(s), o[i] = sum_j a_ij m_ij V[j] per head.  ee is indexed by
    edge id ((n_edges) for 1-D el / er, else (n_edges, h)); m_ij is the multiplier of edge_dropout_mask, 1 at p = 0.
    stats (n_src, h, 2) = (row max, 1 / sum exp) of the undropped scores.  No edge-sized tensor is made."""
    fn = "gat_edge_attention_forward"
    return _gat_attention_forward(fn, row, indptr, eid, indices, el, er, V, negative_slope,
                                  _drop_args(fn, p, seed, offset), ee)


def gat_edge_attention_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, ee, V, o,
                                stats, dO, negative_slope=0.2, p=0.0, seed=0, offset=0, need_dee=True):
    """-> [del, der, dee, dV] of gat_edge_attention_forward for the output gradient dO, with the same (p, seed, offset):
    a and the keep decisions are recomputed per slot from stats.  dee[e] = dz_e in ee's shape is the only edge-sized
    tensor made (edge ids that no row-major slot names get 0); with need_dee=False it is an empty (0,) tensor and
    nothing edge-sized is written."""
    fn = "gat_edge_attention_backward"
    return _gat_attention_backward(fn, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, V, o,
                                   stats, dO, negative_slope, _drop_args(fn, p, seed, offset), ee, need_dee)


# ---- the weights of the fused GAT / GATv2 layers from their row statistics (extra ops) ----------------
def _gat_weights_stats(fn, first, name, stats, h):
    """stats (n_src, h, 2) in the dtype of the row-side operand `first` (el or xl, called `name`)"""
    _same_dtype(first, stats, name, "stats")
    if tuple(stats.shape) != (first.size(0), h, 2):
        raise RuntimeError("%s: stats must be (n_src, h, 2) = (%d, %d, 2), got %s"
                           % (fn, first.size(0), h, tuple(stats.shape)))


def gat_attention_weights(row, indptr, eid, indices, el, er, stats, ee=None, negative_slope=0.2):
    """-> a, the attention weights of gat_attention_forward / gat_attention_dropout_forward (ee=None) or
    gat_edge_attention_forward (ee) from the stats (n_src, h, 2) = (m_i, 1 / l_i) that op returned: for edge e = (i, j),
    s_e = LeakyReLU((el[i] + er[j]) [+ ee[e]]),  a_e = exp(min(s_e - m_i, 0)) / l_i.  a is indexed by edge id, (n_edges)
    for 1-D el / er, else (n_edges, h): the layout of sparse_softmax_forward's result (PyG's
    return_attention_weights=True, DGL's get_attention=True).  These are the UNDROPPED weights; the effective ones are
    a * edge_dropout_mask(...).  The clamp keeps a <= 1 whichever forward produced the statistics.  Edge ids that no
    slot names read 0.  One gather pass: no second softmax, no workspace, no other (n_edges, h) tensor."""
    fn = "gat_attention_weights"
    _check_csr((row, indptr, eid, indices), _CSR, (el, "el"), (er, "er"), (stats, "stats"))
    h = _gat_heads(el, er, fn)
    e = eid.size(0)
    _gat_weights_stats(fn, el, "el", stats, h)
    if ee is not None:
        _gat_edge_term(el, ee, e, h, fn)         # checks ee as an input too
    with _lib.device_guard(el.device):
        plan = get_plan(row, indptr, eid, indices, er.size(0))
        # a[e] is written once per row-major slot: only a chunk list that leaves slots out needs the zeros
        shape = (e,) if el.dim() == 1 else (e, h)
        a = (torch.empty if plan.info.full_coverage else torch.zeros)(shape, dtype=el.dtype, device=el.device)
        check(lib().graphop_gat_attention_weights(
            dtype_code(el), ptr(row), ptr(indptr), ptr(eid), ptr(indices), ptr(el), ptr(er),
            ptr(ee) if ee is not None else _NULL, ptr(stats), ptr(a), row.size(0), e, el.size(0), er.size(0), h,
            float(negative_slope), plan.handle, stream_of(el)))
    return a


def gatv2_attention_weights(row, indptr, eid, indices, xl, xr, att, stats, xe=None, negative_slope=0.2):
    """-> a, the attention weights of gatv2_attention_forward / gatv2_attention_dropout_forward (xe=None, or the edge
    features xe of that call) from the stats (n_src, h, 2) = (m_i, 1 / l_i) that op returned: for edge e = (i, j),
    s_e = att . LeakyReLU((xl[i] + xr[j]) [+ xe[e]]),  a_e = exp(min(s_e - m_i, 0)) / l_i.  a is indexed by edge id,
    (n_edges) for 2-D xl / xr, else (n_edges, h); the UNDROPPED weights, as gat_attention_weights.  One gather pass that
    fetches xr[j] per slot and streams xe once: no second softmax, no workspace, nothing of size (n_edges, h, d)."""
    fn = "gatv2_attention_weights"
    _check_csr((row, indptr, eid, indices), _CSR, (xl, "xl"), (xr, "xr"), (att, "att"), (stats, "stats"))
    h, d = _gatv2_shapes(xl, xr, att, fn)
    e = eid.size(0)
    _gat_weights_stats(fn, xl, "xl", stats, h)
    if xe is not None:
        _gatv2_edge_rows(xl, xe, e, h, d, fn)         # checks xe as an input too
    with _lib.device_guard(xl.device):
        plan = get_plan(row, indptr, eid, indices, xr.size(0))
        shape = (e,) if xl.dim() == 2 else (e, h)
        a = (torch.empty if plan.info.full_coverage else torch.zeros)(shape, dtype=xl.dtype, device=xl.device)
        check(lib().graphop_gatv2_attention_weights(
            dtype_code(xl), ptr(row), ptr(indptr), ptr(eid), ptr(indices), ptr(xl), ptr(xr),
            ptr(xe) if xe is not None else _NULL, ptr(att), ptr(stats), ptr(a), row.size(0), e, xl.size(0), xr.size(0),
            h, d, float(negative_slope), plan.handle, stream_of(xl)))
    return a



def prepare(graph, h=1, d=64, dtype=torch.float32, fused=True):
    """Build a graph's plans and window structures ahead of the first op call (see graphs.prepare)."""
    from . import graphs
    return graphs.prepare(graph, h, d, dtype, fused)


def release(graph):
    """Drop a graph's plans (see graphs.release)."""
    from . import graphs
    graphs.release(graph)


# ---- torch.ops.graphop.* ---------------------------------------------------------------------------
_SCHEMAS = {
    "maskedmm_csr_forward": "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor A, Tensor B) -> Tensor",
    "maskedmm_csr_backward": "(Tensor row, Tensor indptr_r, Tensor eid_r, Tensor indices_r, Tensor col, Tensor indptr_c, Tensor eid_c, Tensor indices_c, Tensor A, Tensor B, Tensor dy) -> Tensor[]",
    "node_mul_edge_forward": "(Tensor row, Tensor indptr, Tensor eid, Tensor A, Tensor B) -> Tensor",
    "node_mul_edge_backward": "(Tensor row, Tensor indptr, Tensor eid, Tensor A, Tensor B, Tensor dy) -> Tensor[]",
    "sparse_softmax_forward": "(Tensor row, Tensor indptr, Tensor eid, Tensor x) -> Tensor",
    "sparse_softmax_backward": "(Tensor row, Tensor indptr, Tensor eid, Tensor y, Tensor dy) -> Tensor",
    "vector_spmm_forward": "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor edata, Tensor x) -> Tensor",
    "vector_spmm_backward": "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor col, Tensor indptr_t, Tensor eid_t, Tensor indices_t, Tensor edata, Tensor dy, Tensor x) -> Tensor[]",
    "attention_forward": "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor Q, Tensor K, Tensor V) -> Tensor[]",
    "attention_backward": "(Tensor row, Tensor indptr_r, Tensor eid_r, Tensor indices_r, Tensor col, Tensor indptr_c, Tensor eid_c, Tensor indices_c, Tensor Q, Tensor K, Tensor V, Tensor o, Tensor stats, Tensor dO) -> Tensor[]",
    "gat_scores_forward": "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor el, Tensor er, float negative_slope=0.2) -> Tensor",
    "gat_scores_backward": "(Tensor row, Tensor indptr_r, Tensor eid_r, Tensor indices_r, Tensor col, Tensor indptr_c, Tensor eid_c, Tensor indices_c, Tensor el, Tensor er, Tensor dy, float negative_slope=0.2) -> Tensor[]",
    "gat_attention_forward": "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor el, Tensor er, Tensor V, float negative_slope=0.2) -> Tensor[]",
    "gat_attention_backward": "(Tensor row, Tensor indptr_r, Tensor eid_r, Tensor indices_r, Tensor col, Tensor indptr_c, Tensor eid_c, Tensor indices_c, Tensor el, Tensor er, Tensor V, Tensor o, Tensor stats, Tensor dO, float negative_slope=0.2) -> Tensor[]",
    "gat_attention_dropout_forward": "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor el, Tensor er, Tensor V, float negative_slope=0.2, float p=0.0, int seed=0, int offset=0) -> Tensor[]",
    "gat_attention_dropout_backward": "(Tensor row, Tensor indptr_r, Tensor eid_r, Tensor indices_r, Tensor col, Tensor indptr_c, Tensor eid_c, Tensor indices_c, Tensor el, Tensor er, Tensor V, Tensor o, Tensor stats, Tensor dO, float negative_slope=0.2, float p=0.0, int seed=0, int offset=0) -> Tensor[]",
    "edge_dropout_mask": "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, int h, float p=0.0, int seed=0, int offset=0, ScalarType dtype=float) -> Tensor",
    "gatv2_scores_forward": "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor xl, Tensor xr, Tensor att, float negative_slope=0.2) -> Tensor",
    "gatv2_scores_backward": "(Tensor row, Tensor indptr_r, Tensor eid_r, Tensor indices_r, Tensor col, Tensor indptr_c, Tensor eid_c, Tensor indices_c, Tensor xl, Tensor xr, Tensor att, Tensor dy, float negative_slope=0.2) -> Tensor[]",
    "gatv2_attention_forward": "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor xl, Tensor xr, Tensor att, float negative_slope=0.2) -> Tensor[]",
    "gatv2_attention_backward": "(Tensor row, Tensor indptr_r, Tensor eid_r, Tensor indices_r, Tensor col, Tensor indptr_c, Tensor eid_c, Tensor indices_c, Tensor xl, Tensor xr, Tensor att, Tensor o, Tensor stats, Tensor dO, float negative_slope=0.2) -> Tensor[]",
    "gatv2_attention_dropout_forward": "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor xl, Tensor xr, Tensor att, float negative_slope=0.2, float p=0.0, int seed=0, int offset=0, Tensor? xe=None) -> Tensor[]",
    "gatv2_attention_dropout_backward": "(Tensor row, Tensor indptr_r, Tensor eid_r, Tensor indices_r, Tensor col, Tensor indptr_c, Tensor eid_c, Tensor indices_c, Tensor xl, Tensor xr, Tensor att, Tensor o, Tensor stats, Tensor dO, float negative_slope=0.2, float p=0.0, int seed=0, int offset=0, Tensor? xe=None, bool need_dxe=True) -> Tensor[]",
    "gat_edge_attention_forward": "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor el, Tensor er, Tensor ee, Tensor V, float negative_slope=0.2, float p=0.0, int seed=0, int offset=0) -> Tensor[]",
    "gat_edge_attention_backward": "(Tensor row, Tensor indptr_r, Tensor eid_r, Tensor indices_r, Tensor col, Tensor indptr_c, Tensor eid_c, Tensor indices_c, Tensor el, Tensor er, Tensor ee, Tensor V, Tensor o, Tensor stats, Tensor dO, float negative_slope=0.2, float p=0.0, int seed=0, int offset=0, bool need_dee=True) -> Tensor[]",
}
# every op beyond the reference's eight, plus the one query that is not an op
# ... and the dropout form of the fused attention step and its forms with a per-edge score bias and with edge features
# (attention_edge_*) and the weights of all of them (attention_weights): bound here and in the compiled extension, not registered under torch.ops.graphop (the registered set is the table above)
EXTRA_OPS = [n for n in _SCHEMAS if n not in __all__] + ["attention_backward_is_fused", "attention_dropout_forward",
                                                         "attention_dropout_backward", "attention_bias_forward",
                                                         "attention_bias_backward", "attention_edge_forward",
                                                         "attention_edge_backward", "attention_weights",
                                                         # edge-type embeddings (attention_etype_*)
                                                         "attention_etype_forward", "attention_etype_backward",
                                                         # an edge-type score bias (attention_tbias_*)
                                                         "attention_tbias_forward", "attention_tbias_backward",
                                                         # the weights of the fused GAT / GATv2 layers
                                                         "gat_attention_weights", "gatv2_attention_weights"]
_torch_lib = None


def _cpu_refusal(name):
    def _impl(*args):
        raise RuntimeError("graphop::%s has no CPU implementation: inputs must be CUDA (ROCm) "
                           "tensors" % name)
    return _impl


cpp_ext = None      # the compiled extension module (csrc/torch_ext.cpp) when it is built, else None


def register_torch_ops():
    """Define torch.ops.graphop.* once.  If the compiled C++ extension graphop_cpp is built, loading
    it registers the namespace from C++ (TORCH_LIBRARY(graphop), csrc/torch_ext.cpp: the reference-style
    boundary over the same C ABI); otherwise the ops are defined here (CUDA key -> the ctypes-bound
    functions above, CPU key -> error)."""
    global _torch_lib, cpp_ext
    if _torch_lib is not None:
        return
    from . import _ext
    cpp_ext = _ext.load()
    if cpp_ext is not None:
        _torch_lib = cpp_ext
        return
    l = torch.library.Library("graphop", "DEF")
    g = globals()
    for name, schema in _SCHEMAS.items():
        l.define(name + schema)
        l.impl(name, g[name], "CUDA")
        l.impl(name, _cpu_refusal(name), "CPU")
    _torch_lib = l


register_torch_ops()
