// GAT additive attention scores (extra op, not in the reference; gat.hip has the entry points):
//   forward : y[eid[j], k] = LeakyReLU(el[row[c], k] + er[indices[j], k], s)      (torch's leaky_relu: z > 0 ? z : z * s)
//   backward: g = dy[e, k] * (z > 0 ? 1 : s), z recomputed from el and er           (torch's leaky_relu_backward)
//             del[row[c], k] += sum of g over the row-major slots, der[col[c], k] += over the column-major slots
// Both backward passes are the same walk with the roles of the two node tables swapped: the chunk's own node row sits
// in registers, the other table is gathered per slot, partial sums stay in registers while the own row is unchanged
// and leave by float atomics only when it changes (one per lane group, row and head: never one per edge).
#pragma once
#include "kernels_base.h"
#include "kernels_generic.h"

namespace graphop {

template <typename T>
__device__ __forceinline__ T gat_lrelu(T z, T s) { return z > (T)0 ? z : z * s; }
template <typename T>
__device__ __forceinline__ T gat_lrelu_grad(T z, T g, T s) { return z > (T)0 ? g : g * s; }

// ---- fp32 fast paths ------------------------------------------------------------------------------
// A slot's H heads are Q = H / 4 float4 items (H >= 4) or one item of H floats (H = 1, 2).  A lane group of G lanes
// takes B = G / Q slots per batch, one item per lane: lane l holds piece q = l % Q of slot l / Q.  The first B lanes
// load the batch's ids (coalesced) and hand them round by shuffles.  A group walks a run of chunks U at a time (U
// independent slot streams in flight per lane), each stream with its own node row in registers.
template <int H>
struct GatCfg {
  static constexpr int Q = H >= 4 ? H / 4 : 1;   // items per slot
  static constexpr int W = H >= 4 ? 4 : H;       // floats per item
  static constexpr int G = H >= 8 ? 64 : 32;     // lanes per group
  static constexpr int B = G / Q;                // slots per batch
  static constexpr int U = 2;                    // chunks in flight per group (4 measured no faster)
};

template <int W>
struct GatItem {
  float v[W];
};

template <int W>
__device__ __forceinline__ GatItem<W> gat_ld(const float* p) {   // p is aligned to 4 * W bytes
  GatItem<W> r;
  if constexpr (W == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else if constexpr (W == 2) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    r.v[0] = t.x; r.v[1] = t.y;
  } else {
    r.v[0] = *p;
  }
  return r;
}

template <int W>
__device__ __forceinline__ void gat_st(float* p, const GatItem<W>& r) {
  if constexpr (W == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  } else if constexpr (W == 2) {
    *reinterpret_cast<float2*>(p) = make_float2(r.v[0], r.v[1]);
  } else {
    *p = r.v[0];
  }
}

template <int H>
__global__ __launch_bounds__(kFastBlock) void k_gat_fwd_f32(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const float* __restrict__ el, const float* __restrict__ er,
    float* __restrict__ y, i64 n_chunks, int chunks_per_group, float s) {
  using C = GatCfg<H>;
  constexpr int Q = C::Q, W = C::W, G = C::G, B = C::B, U = C::U;
  const int l = threadIdx.x % G;
  const int sl = l / Q, q = l % Q;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / G) + threadIdx.x / G;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  GatItem<W> a[U];
  i64 cur[U];
#pragma unroll
  for (int u = 0; u < U; ++u) cur[u] = -1;
  for (i64 c = c0; c < c1; c += U) {
    i64 jb[U];
    int n[U];
    int nmax = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      n[u] = 0;
      jb[u] = 0;
      if (c + u < c1) {
        const i64 r = row[c + u];
        if (r != cur[u]) {
          a[u] = gat_ld<W>(el + r * H + q * W);
          cur[u] = r;
        }
        jb[u] = indptr[c + u];
        n[u] = (int)(indptr[c + u + 1] - jb[u]);
        nmax = n[u] > nmax ? n[u] : nmax;
      }
    }
    for (int off = 0; off < nmax; off += B) {
      int e[U], src[U];
      bool live[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int nb = n[u] - off;
        int my_e = 0, my_s = 0;
        if (l < B && l < nb) {
          my_e = (int)eid[jb[u] + off + l];
          my_s = (int)indices[jb[u] + off + l];
        }
        live[u] = sl < nb;
        e[u] = Q > 1 ? __shfl(my_e, sl, G) : my_e;
        src[u] = Q > 1 ? __shfl(my_s, sl, G) : my_s;
      }
      GatItem<W> b[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (live[u]) b[u] = gat_ld<W>(er + (i64)src[u] * H + q * W);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (live[u]) {
          GatItem<W> o;
#pragma unroll
          for (int i = 0; i < W; ++i) o.v[i] = gat_lrelu(a[u].v[i] + b[u].v[i], s);
          gat_st<W>(y + (i64)e[u] * H + q * W, o);
        }
      }
    }
  }
}

// One backward pass: seg[c] names the chunk's own node (row of el for the row pass, column of er for the column pass),
// `own` is that table, `oth` the gathered one, out[seg[c]] += the pass's gradient.
template <int H>
__device__ __forceinline__ void gat_bwd_walk(
    const i64* __restrict__ seg, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const float* __restrict__ own, const float* __restrict__ oth,
    const float* __restrict__ dy, float* __restrict__ out, i64 n_chunks, int chunks_per_group, float s) {
  using C = GatCfg<H>;
  constexpr int Q = C::Q, W = C::W, G = C::G, B = C::B, U = C::U;
  const int l = threadIdx.x % G;
  const int sl = l / Q, q = l % Q;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / G) + threadIdx.x / G;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  GatItem<W> a[U], acc[U];
  i64 cur[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    cur[u] = -1;
#pragma unroll
    for (int i = 0; i < W; ++i) acc[u].v[i] = 0.f;
  }
  // group-uniform: every lane of the group takes part in the reduction; the lanes of slot 0 add the Q items
  auto flush = [&](int u) {
#pragma unroll
    for (int i = 0; i < W; ++i) {
      float v = acc[u].v[i];
#pragma unroll
      for (int o = Q; o < G; o <<= 1) v += __shfl_xor(v, o, G);
      if (sl == 0) atomicAdd(out + cur[u] * H + q * W + i, v);
      acc[u].v[i] = 0.f;
    }
  };
  for (i64 c = c0; c < c1; c += U) {
    i64 jb[U];
    int n[U];
    int nmax = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      n[u] = 0;
      jb[u] = 0;
      if (c + u < c1) {
        const i64 r = seg[c + u];
        if (r != cur[u]) {
          if (cur[u] >= 0) flush(u);
          a[u] = gat_ld<W>(own + r * H + q * W);
          cur[u] = r;
        }
        jb[u] = indptr[c + u];
        n[u] = (int)(indptr[c + u + 1] - jb[u]);
        nmax = n[u] > nmax ? n[u] : nmax;
      }
    }
    for (int off = 0; off < nmax; off += B) {
      int e[U], src[U];
      bool live[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int nb = n[u] - off;
        int my_e = 0, my_s = 0;
        if (l < B && l < nb) {
          my_e = (int)eid[jb[u] + off + l];
          my_s = (int)indices[jb[u] + off + l];
        }
        live[u] = sl < nb;
        e[u] = Q > 1 ? __shfl(my_e, sl, G) : my_e;
        src[u] = Q > 1 ? __shfl(my_s, sl, G) : my_s;
      }
      GatItem<W> b[U], g[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (live[u]) {
          b[u] = gat_ld<W>(oth + (i64)src[u] * H + q * W);
          g[u] = gat_ld<W>(dy + (i64)e[u] * H + q * W);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (live[u]) {
#pragma unroll
          for (int i = 0; i < W; ++i) acc[u].v[i] += gat_lrelu_grad(a[u].v[i] + b[u].v[i], g[u].v[i], s);
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (cur[u] >= 0) flush(u);
}

// row pass: del[row[c]] over the row-major chunks (el in registers, er gathered, dy streamed by eid_r)
template <int H>
__global__ __launch_bounds__(kFastBlock) void k_gat_bwd_row_f32(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const float* __restrict__ el, const float* __restrict__ er,
    const float* __restrict__ dy, float* __restrict__ del, i64 n_chunks, int chunks_per_group, float s) {
  gat_bwd_walk<H>(row, indptr, eid, indices, el, er, dy, del, n_chunks, chunks_per_group, s);
}

// column pass: der[col[c]] over the column-major chunks (er in registers, el and dy[eid_c] gathered)
template <int H>
__global__ __launch_bounds__(kFastBlock) void k_gat_bwd_col_f32(
    const i64* __restrict__ col, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const float* __restrict__ el, const float* __restrict__ er,
    const float* __restrict__ dy, float* __restrict__ der, i64 n_chunks, int chunks_per_group, float s) {
  gat_bwd_walk<H>(col, indptr, eid, indices, er, el, dy, der, n_chunks, chunks_per_group, s);
}

// ---- generic kernels: any h, fp32 or fp64, any chunk layout; one wave per chunk ------------------------
template <typename T>
__global__ __launch_bounds__(kGenericBlock) void k_gat_fwd_generic(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ el, const T* __restrict__ er, T* __restrict__ y,
    i64 n_chunks, i64 h, T s) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = row[c];
  const i64 j0 = indptr[c];
  const i64 items = (indptr[c + 1] - j0) * h;
  for (i64 it = lane; it < items; it += kWave) {
    const i64 j = j0 + it / h, k = it % h;
    y[eid[j] * h + k] = gat_lrelu(el[r * h + k] + er[indices[j] * h + k], s);
  }
}

// Lanes are (slot, head) pairs when h divides the wave (hp = h heads at a time), else one head at a time (hp = 1);
// a lane's partial sum stays on one head, the wave reduces over the lanes of a head and adds once per chunk and head.
template <typename T>
__device__ __forceinline__ void gat_bwd_generic(
    const i64* __restrict__ seg, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ own, const T* __restrict__ oth, const T* __restrict__ dy,
    T* __restrict__ out, i64 n_chunks, i64 h, T s) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = seg[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  const int hp = (h <= kWave && kWave % h == 0) ? (int)h : 1;
  const int spw = kWave / hp;   // slots per wave step
  for (i64 kb = 0; kb < h; kb += hp) {
    const i64 k = kb + lane % hp;
    const T a = own[r * h + k];
    T acc = 0;
    for (i64 j = j0 + lane / hp; j < j1; j += spw)
      acc += gat_lrelu_grad(a + oth[indices[j] * h + k], dy[eid[j] * h + k], s);
    for (int o = hp; o < kWave; o <<= 1) acc += __shfl_xor(acc, o);
    if (lane < hp && j1 > j0) atomicAdd(out + r * h + k, acc);
  }
}

template <typename T>
__global__ __launch_bounds__(kGenericBlock) void k_gat_bwd_row_generic(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ el, const T* __restrict__ er, const T* __restrict__ dy,
    T* __restrict__ del, i64 n_chunks, i64 h, T s) {
  gat_bwd_generic<T>(row, indptr, eid, indices, el, er, dy, del, n_chunks, h, s);
}

template <typename T>
__global__ __launch_bounds__(kGenericBlock) void k_gat_bwd_col_generic(
    const i64* __restrict__ col, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ el, const T* __restrict__ er, const T* __restrict__ dy,
    T* __restrict__ der, i64 n_chunks, i64 h, T s) {
  gat_bwd_generic<T>(col, indptr, eid, indices, er, el, dy, der, n_chunks, h, s);
}

}  // namespace graphop
