"""Pure-torch reference of the GAT additive attention scores and of the GAT attention layer built on them
(graphop.gat_scores_forward / _backward, functions.GATScores, functions.gat_attention_step).  CPU, autograd-able."""
import torch
import torch.nn.functional as F


def gat_scores(src, dst, el, er, negative_slope):
    """s[e, k] = LeakyReLU(el[src[e], k] + er[dst[e], k]): (E) for 1-D el / er, else (E, h)."""
    return F.leaky_relu(el[src] + er[dst], negative_slope)


def gat_layer(src, dst, n_out, el, er, V, negative_slope):
    """o[i] = sum_j a_ij V[j], a = softmax over the edges (i, j) of row i of the scores; segment max by scatter_reduce,
    sums by index_add.  V is (n, d) with 1-D el / er, else (n, h, d)."""
    s = gat_scores(src, dst, el, er, negative_slope)
    s2 = s if s.dim() == 2 else s[:, None]
    h = s2.size(1)
    idx = src[:, None].expand(-1, h)
    m = torch.full((n_out, h), float("-inf"), dtype=s2.dtype).scatter_reduce(0, idx, s2.detach(), "amax")
    ex = torch.exp(s2 - m[src])
    den = torch.zeros((n_out, h), dtype=s2.dtype).index_add(0, src, ex)
    a = ex / den[src]
    V3 = V if V.dim() == 3 else V[:, None, :]
    o = torch.zeros((n_out, h, V3.size(-1)), dtype=V.dtype).index_add(0, src, a[..., None] * V3[dst])
    return o if V.dim() == 3 else o[:, 0, :]


def reorder_chunks(indptr, row, eid, indices, order):
    """The chunk list (row, indptr) over (eid, indices) with its chunks taken in `order` (a permutation, or a subset to
    leave some slots uncovered): slot arrays rebuilt so that every chunk is again one contiguous slot range."""
    starts, ends = indptr[:-1][order], indptr[1:][order]
    slots = torch.cat([torch.arange(int(a), int(b)) for a, b in zip(starts, ends)] or [torch.zeros(0, dtype=torch.int64)])
    lens = ends - starts
    new_ptr = torch.zeros(len(order) + 1, dtype=torch.int64)
    new_ptr[1:] = torch.cumsum(lens, 0)
    return new_ptr, row[order].clone(), eid[slots].clone(), indices[slots].clone()
