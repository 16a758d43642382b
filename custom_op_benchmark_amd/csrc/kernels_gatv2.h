// GATv2 attention scores (extra op, not in the reference; gatv2.hip has the entry points):
//   forward : y[eid[j], k] = sum_c att[k, c] * LeakyReLU(xl[row[c], k, c] + xr[indices[j], k, c], s)
//   backward: g[e, k, c] = dy[e, k] * att[k, c] * (z > 0 ? 1 : s), z recomputed from xl and xr (the tie takes s)
//             dxl[row[c]] += sum of g over the row-major slots, dxr[col[c]] += over the column-major slots,
//             datt[k, c]  = sum over the row-major slots of dy[e, k] * LeakyReLU(z[e, k, c])
// fp32 fast forms (the chunk driver of kernels_gat_attn.h's backward passes): a node row of H * D floats is
// F4 = H * D / 4 float4 pieces; a lane group of L = 16 lanes holds NV = F4 / L of them, piece p = v * L + l, so the
// DQ = D / 4 pieces of one head sit in DQ adjacent lanes and a per-head sum is a group_sum<DQ>.  The chunk's own node
// row and the lane's pieces of att stay in registers; neighbour ids are loaded by the first lanes of the group and handed
// round by group_bcast; SB gathered rows are in flight per lane.  Row gradients leave once per (lane group, row): stored
// where the group owns the row, added by float atomics where a row is split.  datt stays in registers for the group's
// whole run of chunks and leaves once per workgroup as a row of per-block partials (k_gatv2_datt_fin_f32 sums them in
// a fixed order: datt is reproducible bit for bit).  k_gatv2_*_generic<T> cover fp64, other shapes, NULL plans and any
// chunk order.
#pragma once
#include "kernels_base.h"
#include "kernels_gat.h"
#include "kernels_generic.h"

namespace graphop {

template <int H, int D>
struct Gatv2Cfg {
  static constexpr int L = 16;               // lanes per group
  static constexpr int F4 = H * D / 4;       // float4 pieces of a node row
  static constexpr int NV = F4 / L;          // pieces per lane (1, 2, 4)
  static constexpr int DQ = D / 4;           // lanes holding one head's pieces (2 .. 16)
  static constexpr int SB_FWD = 16 / NV;     // slots per batch: 16 gathered float4 pieces in flight per lane
  static constexpr int SB_BWD = 8 / NV;      // the backward passes also keep a row of sums (two in the row pass)
  static_assert(NV * L == F4 && DQ <= L && L % DQ == 0, "unsupported (H, D)");
};

// sum_i w_i * LeakyReLU(a_i + b_i) over the four components of a piece
__device__ __forceinline__ float gatv2_dot4(const float4& w, const float4& a, const float4& b, float s) {
  return fmaf(w.w, gat_lrelu(a.w + b.w, s),
              fmaf(w.z, gat_lrelu(a.z + b.z, s), fmaf(w.y, gat_lrelu(a.y + b.y, s), w.x * gat_lrelu(a.x + b.x, s))));
}

// ---- forward ---------------------------------------------------------------------------------------------------------
// One score per (slot, head), stored by the first lane of the head's DQ lanes; for H = 1 the batch's scores are
// collected across the group and leave in one store instruction.
template <int H, int D>
__global__ __launch_bounds__(kFastBlock) void k_gatv2_fwd_f32(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const float* __restrict__ xl, const float* __restrict__ xr,
    const float* __restrict__ att, float* __restrict__ y, i64 n_chunks, int chunks_per_group, float slope) {
  using C = Gatv2Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB_FWD;
  constexpr i64 F4 = C::F4;
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  if (c0 >= c1) return;
  int kv[NV];
  float4 w[NV], a[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    kv[v] = (v * L + l) / DQ;
    w[v] = ld4(att, v * L + l);
  }
  i64 cur = -1;
  for (i64 c = c0; c < c1; ++c) {
    const i64 r = row[c];
    if (r != cur) {
      cur = r;
#pragma unroll
      for (int v = 0; v < NV; ++v) a[v] = ld4(xl, r * F4 + v * L + l);
    }
    const i64 j0 = indptr[c], j1 = indptr[c + 1];
    for (i64 jb = j0; jb < j1; jb += SB) {
      const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
      int my_src = 0, my_e = 0;   // slots past the end re-read the batch's last neighbour; nothing is stored for them
      if (l < SB) {
        const i64 j = jb + (l < nb ? l : nb - 1);
        my_src = (int)indices[j];
        my_e = (int)eid[j];
      }
      float4 x[SB][NV];
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
#pragma unroll
        for (int v = 0; v < NV; ++v) x[u][v] = ld4(xr, src * F4 + v * L + l);
      });
      float res = 0.f;
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        if constexpr (H == 1) {
          float p = 0.f;
#pragma unroll
          for (int v = 0; v < NV; ++v) p += gatv2_dot4(w[v], a[v], x[u][v], slope);
          p = group_sum<L>(p);
          if (l == u) res = p;
        } else {
          const i64 e = group_bcast<L, u>(my_e);
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            const float p = group_sum<DQ>(gatv2_dot4(w[v], a[v], x[u][v], slope));
            if (u < nb && l % DQ == 0) y[e * H + kv[v]] = p;
          }
        }
      });
      if constexpr (H == 1) {
        if (l < nb) y[my_e] = res;
      }
    }
  }
}

// ---- backward passes -------------------------------------------------------------------------------------------------
// seg[c] names the chunk's own node (row of xl for the row pass, column of xr for the column pass), `own` is that
// table, `oth` the gathered one, out[seg[c]] += the pass's gradient.  DATT (the row pass): the lane's pieces of datt are
// summed over the group's whole run, reduced over the workgroup (shuffles inside a wave, LDS across waves) and written
// as row blockIdx.x of datt_part (gridDim.x, F4): every workgroup writes its row, groups without chunks add zeros.
// att does not depend on the slot: a row's sum is kept as sum_j dy * (z > 0 ? 1 : s) and multiplied by the lane's pieces
// of att when it leaves (read there, once per row and group, so that they hold no registers inside the slot loop).
template <int H, int D, bool DATT, bool OWNED>
__device__ __forceinline__ void gatv2_bwd_walk(
    const i64* __restrict__ seg, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const float* __restrict__ own, const float* __restrict__ oth,
    const float* __restrict__ att, const float* __restrict__ dy, float* __restrict__ out,
    float4* __restrict__ datt_part, i64 n_chunks, int chunks_per_group, float slope) {
  using C = Gatv2Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB_BWD;
  constexpr i64 F4 = C::F4;
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  int kv[NV];
  float4 a[NV], acc[NV], dw[DATT ? NV : 1];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    kv[v] = (v * L + l) / DQ;
    acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int v = 0; v < (DATT ? NV : 1); ++v) dw[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c0 < c1) {   // group-uniform
    i64 row_before = -1, row_after = -1;
    if constexpr (OWNED) {
      if (c0 > 0) row_before = seg[c0 - 1];
      if (c1 < n_chunks) row_after = seg[c1];
    }
    auto flush = [&](i64 r) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const float4 w = ld4(att, v * L + l);
        acc[v].x *= w.x; acc[v].y *= w.y; acc[v].z *= w.z; acc[v].w *= w.w;
      }
      if (OWNED && r != row_before && r != row_after) {
#pragma unroll
        for (int v = 0; v < NV; ++v) reinterpret_cast<float4*>(out)[r * F4 + v * L + l] = acc[v];
      } else {
        atomic_flush<L, NV>(out, r, acc, l);
      }
#pragma unroll
      for (int v = 0; v < NV; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    };
    i64 cur = -1;
    bool dirty = false;
    for (i64 c = c0; c < c1; ++c) {
      const i64 r = seg[c];
      if (r != cur) {
        if (dirty) { flush(cur); dirty = false; }
        cur = r;
#pragma unroll
        for (int v = 0; v < NV; ++v) a[v] = ld4(own, r * F4 + v * L + l);
      }
      const i64 j0 = indptr[c], j1 = indptr[c + 1];
      if (j1 > j0) dirty = true;
      for (i64 jb = j0; jb < j1; jb += SB) {
        const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
        int my_src = 0, my_e = 0;   // slots past the end re-read the batch's last slot with dy = 0
        float my_g = 0.f;
        if (l < SB) {
          const i64 j = jb + (l < nb ? l : nb - 1);
          my_src = (int)indices[j];
          my_e = (int)eid[j];
          if constexpr (H == 1) my_g = dy[my_e];
        }
        float4 x[SB][NV];
        float g[SB][NV];
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          const i64 src = group_bcast<L, u>(my_src);
#pragma unroll
          for (int v = 0; v < NV; ++v) x[u][v] = ld4(oth, src * F4 + v * L + l);
          if constexpr (H == 1) {
            const float t = group_bcast<L, u>(my_g);
#pragma unroll
            for (int v = 0; v < NV; ++v) g[u][v] = t;
          } else {
            const i64 e = group_bcast<L, u>(my_e);
#pragma unroll
            for (int v = 0; v < NV; ++v) g[u][v] = dy[e * H + kv[v]];
          }
        });
#pragma unroll
        for (int u = 0; u < SB; ++u) {
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            const float gd = u < nb ? g[u][v] : 0.f;
            const float zx = a[v].x + x[u][v].x, zy = a[v].y + x[u][v].y;
            const float zz = a[v].z + x[u][v].z, zw = a[v].w + x[u][v].w;
            const float gs = gd * slope;
            acc[v].x += zx > 0.f ? gd : gs;
            acc[v].y += zy > 0.f ? gd : gs;
            acc[v].z += zz > 0.f ? gd : gs;
            acc[v].w += zw > 0.f ? gd : gs;
            if constexpr (DATT) {
              dw[v].x = fmaf(gd, gat_lrelu(zx, slope), dw[v].x);
              dw[v].y = fmaf(gd, gat_lrelu(zy, slope), dw[v].y);
              dw[v].z = fmaf(gd, gat_lrelu(zz, slope), dw[v].z);
              dw[v].w = fmaf(gd, gat_lrelu(zw, slope), dw[v].w);
            }
          }
        }
      }
    }
    if (dirty) flush(cur);
  }
  if constexpr (DATT) {   // every thread of the workgroup arrives here
    static_assert(F4 <= kWave, "one thread per piece in the last step");
    __shared__ float4 red[kFastBlock / kWave][F4];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      float4 t = dw[v];
#pragma unroll
      for (int o = L; o < kWave; o <<= 1) {
        t.x += __shfl_xor(t.x, o); t.y += __shfl_xor(t.y, o);
        t.z += __shfl_xor(t.z, o); t.w += __shfl_xor(t.w, o);
      }
      if (lane < L) red[wv][v * L + lane] = t;
    }
    __syncthreads();
    if (threadIdx.x < F4) {
      float4 t = red[0][threadIdx.x];
#pragma unroll
      for (int q = 1; q < kFastBlock / kWave; ++q) {
        const float4 o = red[q][threadIdx.x];
        t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
      }
      datt_part[(i64)blockIdx.x * F4 + threadIdx.x] = t;
    }
  }
}

// row pass: dxl[row[c]] and datt over the row-major chunks (xl in registers, xr gathered, dy read by eid_r); compiled for
// four workgroups per CU (128 VGPRs at most: the widest instantiations sit within fifteen registers of that line)
template <int H, int D, bool OWNED>
__global__ __launch_bounds__(kFastBlock, 4) void k_gatv2_bwd_row_f32(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const float* __restrict__ xl, const float* __restrict__ xr,
    const float* __restrict__ att, const float* __restrict__ dy, float* __restrict__ dxl,
    float4* __restrict__ datt_part, i64 n_chunks, int chunks_per_group, float slope) {
  gatv2_bwd_walk<H, D, true, OWNED>(row, indptr, eid, indices, xl, xr, att, dy, dxl, datt_part, n_chunks,
                                    chunks_per_group, slope);
}

// column pass: dxr[col[c]] over the column-major chunks (xr in registers, xl and dy[eid_c] gathered)
template <int H, int D, bool OWNED>
__global__ __launch_bounds__(kFastBlock) void k_gatv2_bwd_col_f32(
    const i64* __restrict__ col, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const float* __restrict__ xl, const float* __restrict__ xr,
    const float* __restrict__ att, const float* __restrict__ dy, float* __restrict__ dxr, i64 n_chunks,
    int chunks_per_group, float slope) {
  gatv2_bwd_walk<H, D, false, OWNED>(col, indptr, eid, indices, xr, xl, att, dy, dxr, nullptr, n_chunks,
                                     chunks_per_group, slope);
}

// datt[p] = sum over the n_part rows of the row pass's partials, piece p = blockIdx.x: each thread sums its rows in
// order, then the workgroup's 256 sums are added in a fixed tree
__global__ __launch_bounds__(kFastBlock) void k_gatv2_datt_fin_f32(const float4* __restrict__ part,
                                                                   float4* __restrict__ datt, i64 n_part, int f4) {
  __shared__ float4 red[kFastBlock / kWave];
  const int p = blockIdx.x;
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
  for (i64 i = threadIdx.x; i < n_part; i += kFastBlock) {
    const float4 o = part[i * f4 + p];
    t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
  }
  t.x = wave_sum(t.x); t.y = wave_sum(t.y); t.z = wave_sum(t.z); t.w = wave_sum(t.w);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 1; q < kFastBlock / kWave; ++q) {
      t.x += red[q].x; t.y += red[q].y; t.z += red[q].z; t.w += red[q].w;
    }
    datt[p] = t;
  }
}

// ---- generic kernels: any h and d, fp32 or fp64, any chunk layout; one wave per chunk ---------------------------------
// forward: dp = the power of two that covers d (64 at most) lanes take one head, kWave / dp heads at a time; a lane
// sums its c = lane % dp, + dp, ... and the head's dp lanes are reduced by shuffles, once per (slot, head)
template <typename T>
__global__ __launch_bounds__(kGenericBlock) void k_gatv2_fwd_generic(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ xl, const T* __restrict__ xr, const T* __restrict__ att,
    T* __restrict__ y, i64 n_chunks, i64 h, i64 d, int dp, T s) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = row[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  const int hp = kWave / dp, kk = lane / dp, cc = lane % dp;
  for (i64 kb = 0; kb < h; kb += hp) {   // wave-uniform trip counts: every lane takes part in the shuffles
    const i64 k = kb + kk;
    const bool on = k < h;
    for (i64 j = j0; j < j1; ++j) {
      const i64 n = indices[j];
      T p = 0;
      if (on)
        for (i64 ci = cc; ci < d; ci += dp)
          p += att[k * d + ci] * gat_lrelu(xl[(r * h + k) * d + ci] + xr[(n * h + k) * d + ci], s);
      for (int o = 1; o < dp; o <<= 1) p += __shfl_xor(p, o);
      if (on && cc == 0) y[eid[j] * h + k] = p;
    }
  }
}

// backward: lanes over the h * d elements of the own row in steps of the wave; a lane's element keeps its sums over
// the chunk's slots in registers and adds them once: one atomic per (chunk, element) into out, and into datt (DATT)
template <typename T, bool DATT>
__device__ __forceinline__ void gatv2_bwd_generic(
    const i64* __restrict__ seg, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ own, const T* __restrict__ oth, const T* __restrict__ att,
    const T* __restrict__ dy, T* __restrict__ out, T* __restrict__ datt, i64 n_chunks, i64 h, i64 d, T s) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = seg[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  if (j1 <= j0) return;
  const i64 f = h * d;
  for (i64 it = lane; it < f; it += kWave) {
    const i64 k = it / d;
    const T a = own[r * f + it], w = att[it];
    T acc = 0, dw = 0;
    for (i64 j = j0; j < j1; ++j) {
      const T g = dy[eid[j] * h + k];
      const T z = a + oth[indices[j] * f + it];
      acc += gat_lrelu_grad(z, g * w, s);
      if constexpr (DATT) dw += g * gat_lrelu(z, s);
    }
    atomicAdd(out + r * f + it, acc);
    if constexpr (DATT) atomicAdd(datt + it, dw);
  }
}

template <typename T>
__global__ __launch_bounds__(kGenericBlock) void k_gatv2_bwd_row_generic(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ xl, const T* __restrict__ xr, const T* __restrict__ att,
    const T* __restrict__ dy, T* __restrict__ dxl, T* __restrict__ datt, i64 n_chunks, i64 h, i64 d, T s) {
  gatv2_bwd_generic<T, true>(row, indptr, eid, indices, xl, xr, att, dy, dxl, datt, n_chunks, h, d, s);
}

template <typename T>
__global__ __launch_bounds__(kGenericBlock) void k_gatv2_bwd_col_generic(
    const i64* __restrict__ col, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ xl, const T* __restrict__ xr, const T* __restrict__ att,
    const T* __restrict__ dy, T* __restrict__ dxr, i64 n_chunks, i64 h, i64 d, T s) {
  gatv2_bwd_generic<T, false>(col, indptr, eid, indices, xr, xl, att, dy, dxr, nullptr, n_chunks, h, d, s);
}

}  // namespace graphop
