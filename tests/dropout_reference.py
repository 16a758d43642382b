"""CPU statement of the attention dropout of the fused GAT layer (include/graphop_hip.h): Philox4x32-10
in numpy, the keep decision of edge (i, j) and head k, the multipliers m_ijk as an edge tensor, and the GAT layer with
dropout built like gat_reference.gat_layer (autograd-able).

    w[0..3] = Philox4x32-10(counter = (i, j, k >> 2, offset), key = (seed & 0xffffffff, seed >> 32))
    keep(i, j, k) = w[k & 3] >= T,  T = floor(p * 2^32);  m_ijk = keep ? 1 / (1 - p) : 0

i is the row-major row id (src, the index into el / o), j the neighbour id (dst, the index into er / V)."""
import math

import numpy as np
import torch

from gat_reference import gat_scores

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints or arrays -> (..., 4) uint32."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK) for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(x, dtype=np.uint64) & np.uint64(MASK) for x in key)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(W0)) & np.uint64(MASK)
        k1 = (k1 + np.uint64(W1)) & np.uint64(MASK)
    return np.stack(c, axis=-1).astype(np.uint32)


def threshold(p):
    """T = floor(p * 2^32), in double"""
    return int(math.floor(float(p) * 4294967296.0))


def keep(src, dst, h, p, seed, offset=0):
    """(E, h) bool numpy array: keep(i = src[e], j = dst[e], k)"""
    src = np.asarray(src, dtype=np.uint64)
    dst = np.asarray(dst, dtype=np.uint64)
    seed = int(seed)
    assert 0 <= p < 1 and 0 <= seed < 2 ** 63 and 0 <= offset < 2 ** 32
    out = np.empty((src.shape[0], h), dtype=bool)
    for b in range((h + 3) // 4):
        w = philox4x32_10((src, dst, b, offset), (seed & MASK, seed >> 32))
        n = min(4, h - 4 * b)
        out[:, 4 * b:4 * b + n] = w[:, :n].astype(np.uint64) >= np.uint64(threshold(p))
    return out


def multipliers(src, dst, h, p, seed, offset=0, dtype=torch.float64):
    """m[e, k] = keep ? 1 / (1 - p) : 0 with 1 / (1 - p) computed in double and rounded to dtype: (E, h)"""
    scale = torch.tensor(1.0 / (1.0 - float(p)), dtype=torch.float64).to(dtype)
    k = torch.from_numpy(keep(src, dst, h, p, seed, offset))
    return torch.where(k, scale, torch.zeros((), dtype=dtype))


def gat_layer_dropout(src, dst, n_out, el, er, V, negative_slope, p, seed, offset=0):
    """o[i] = sum_j a_ij m_ij V[j]: gat_reference.gat_layer with the weights masked and rescaled after the softmax (the
    row statistics are those of the undropped scores).  V is (n, d) with 1-D el / er, else (n, h, d)."""
    s = gat_scores(src, dst, el, er, negative_slope)
    s2 = s if s.dim() == 2 else s[:, None]
    h = s2.size(1)
    idx = src[:, None].expand(-1, h)
    m = torch.full((n_out, h), float("-inf"), dtype=s2.dtype).scatter_reduce(0, idx, s2.detach(), "amax")
    ex = torch.exp(s2 - m[src])
    den = torch.zeros((n_out, h), dtype=s2.dtype).index_add(0, src, ex)
    a = ex / den[src] * multipliers(src.numpy(), dst.numpy(), h, p, seed, offset, s2.dtype)
    V3 = V if V.dim() == 3 else V[:, None, :]
    o = torch.zeros((n_out, h, V3.size(-1)), dtype=V.dtype).index_add(0, src, a[..., None] * V3[dst])
    return o if V.dim() == 3 else o[:, 0, :]


def fully_dropped_rows(src, dst, n_out, h, p, seed, offset=0):
    """(n_out, h) bool tensor: rows with at least one edge whose every edge is dropped for that head"""
    k = torch.from_numpy(keep(src.numpy(), dst.numpy(), h, p, seed, offset))
    kept = torch.zeros((n_out, h), dtype=torch.int64).index_add(0, src, k.long())
    deg = torch.zeros(n_out, dtype=torch.int64).index_add(0, src, torch.ones_like(src))
    return (deg[:, None] > 0) & (kept == 0)
