// Fused attention with a per-edge score bias (graphop_attention_bias_*):
//   s_e = <Q_i, K_j> + b[e]   for edge e = (i, j), b indexed by EDGE ID, one add after the dot product's reduction
//   a_e = exp(s_e - m_i) * linv_i,   o_i = sum_e a_e m_e V_j   (m_e: the dropout multiplier, 1 without DROP)
//   ds_e = a_e (m_e <dO_i, V_j> - D_i),   db[e] = ds_e;   dQ, dK, dV from ds_e and a_e m_e as without the bias
// Here: the elementwise add of the composed path and the chunk-driver form of the two backward passes.  The backward
// kernel is k_attn_bwd_rows_f32 (kernels_attn.h) restated with the three additions the bias needs -- that kernel keeps
// its text, its template arguments and its registers (tests/test_attention_dropout_host.py pins them), so nothing is
// shared with it but the helpers.  The lane l < nb that owns slot jb + l loads b[e], e = eid[jb + l] (a NULL eid means
// eid[slot] == slot: a row-major plan with eid_identity), behind the row requests, adds it to its reduced score and,
// in the row pass with db given, stores db[e] = ds: every edge is one row-major slot, so the stores are plain.
#pragma once
#include "kernels_attn.h"

namespace graphop {

// s[i] += b[i] over the n = n_edges * h values; both arrays are indexed by edge id
template <typename T>
__global__ void k_attn_bias_add(T* __restrict__ s, const T* __restrict__ b, i64 n) {
  i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (; i < n; i += stride) s[i] += b[i];
}

//   COL = false: OWN = (Q | dO) packed [n_q][2F], XT = (K | V) packed, out0 = dQ; db (may be NULL) is written
//   COL = true : OWN = (K | V) packed [n_k][2F], XT = (Q | dO) packed, out0 = dK, out1 = dV; db is not touched
template <int L, int NV, bool COL, bool OWNED, bool DROP>
__global__ __launch_bounds__(kFastBlock) void k_attn_bias_bwd_rows_f32(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const float* __restrict__ OWN, const float* __restrict__ XT,
    const float4* __restrict__ stats4, const float* __restrict__ b, float* __restrict__ out0, float* __restrict__ out1,
    float* __restrict__ db, i64 n_chunks, int chunks_per_group, AttnDropIf<DROP> dr) {
  constexpr int SB = AttnCfg<L, NV>::SB;
  constexpr i64 F4 = (i64)L * NV;
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * GroupCfg<L>::kGroupsPerBlock + threadIdx.x / L;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  if (c0 >= c1) return;
  i64 row_before = -1, row_after = -1;
  if constexpr (OWNED) {
    if (c0 > 0) row_before = row[c0 - 1];
    if (c1 < n_chunks) row_after = row[c1];
  }
  float4 y0[NV], y1[NV], acc0[NV], acc1[COL ? NV : 1];
  float4 own_st = make_float4(0.f, 0.f, 0.f, 0.f);
  auto zero_acc = [&]() {
#pragma unroll
    for (int v = 0; v < NV; ++v) acc0[v] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int v = 0; v < (COL ? NV : 1); ++v) acc1[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto flush = [&](i64 r) {
    if (OWNED && r != row_before && r != row_after) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        reinterpret_cast<float4*>(out0)[r * F4 + v * L + l] = acc0[v];
        if constexpr (COL) reinterpret_cast<float4*>(out1)[r * F4 + v * L + l] = acc1[v];
      }
    } else {
      atomic_flush<L, NV>(out0, r, acc0, l);
      if constexpr (COL) atomic_flush<L, NV>(out1, r, acc1, l);
    }
  };
  zero_acc();
  i64 cur_row = -1;
  bool dirty = false;
  for (i64 c = c0; c < c1; ++c) {
    const i64 r = row[c];
    if (r != cur_row) {
      if (dirty) { flush(cur_row); zero_acc(); dirty = false; }
      cur_row = r;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        y0[v] = ld4(OWN, r * 2 * F4 + v * L + l);
        y1[v] = ld4(OWN, r * 2 * F4 + F4 + v * L + l);
      }
      if constexpr (!COL) own_st = stats4[r];
    }
    const i64 j0 = indptr[c], j1 = indptr[c + 1];
    if (j1 > j0) dirty = true;
    for (i64 jb = j0; jb < j1; jb += SB) {
      const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
      // slots past the end re-read the batch's last neighbour with weights 0
      i64 my_src = 0;
      float4 st = own_st;
      if (l < SB) {
        my_src = indices[jb + (l < nb ? l : nb - 1)];
        if constexpr (COL) st = stats4[my_src];
      }
      float mult = 1.f;
      if constexpr (DROP) {   // lane u < nb holds slot u's ids: one Philox call per batch
        if (l < nb) mult = COL ? attn_drop_mult((unsigned)my_src, (unsigned)cur_row, dr)
                               : attn_drop_mult((unsigned)cur_row, (unsigned)my_src, dr);
      }
      float4 x0[SB][NV], x1[SB][NV];
#pragma unroll
      for (int u = 0; u < SB; ++u) {
        const i64 src = __shfl(my_src, u, L);
        const float4* rowp = reinterpret_cast<const float4*>(XT) + src * (2 * F4) + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) { x0[u][v] = rowp[v * L]; x1[u][v] = rowp[F4 + v * L]; }
      }
      // the slot's edge id and bias (issued behind the row requests)
      i64 my_e = 0;
      float my_b = 0.f;
      if (l < nb) {
        my_e = eid ? eid[jb + l] : jb + l;   // kernel-uniform branch
        my_b = b[my_e];
      }
      float my_s = 0.f, my_da = 0.f;
#pragma unroll
      for (int u = 0; u < SB; ++u) {
        float p = dot4(y0[0], x0[u][0]), q = dot4(y1[0], x1[u][0]);
#pragma unroll
        for (int v = 1; v < NV; ++v) { p += dot4(y0[v], x0[u][v]); q += dot4(y1[v], x1[u][v]); }
        p = group_sum<L>(p);
        q = group_sum<L>(q);
        if (l == u) { my_s = p; my_da = q; }
      }
      float a_l = 0.f, ds_l = 0.f;
      if (l < nb) {
        my_s += my_b;
        a_l = expf(my_s - st.x) * st.y;
        if constexpr (DROP) my_da *= mult;
        ds_l = a_l * (my_da - st.z);
        if constexpr (DROP && COL) a_l *= mult;   // from here on a_l only weights dV
        if constexpr (!COL) {
          if (db != nullptr) db[my_e] = ds_l;     // kernel-uniform check: the gradient of b is wanted
        }
      }
#pragma unroll
      for (int u = 0; u < SB; ++u) {
        const float dsu = __shfl(ds_l, u, L);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          acc0[v].x = fmaf(dsu, x0[u][v].x, acc0[v].x); acc0[v].y = fmaf(dsu, x0[u][v].y, acc0[v].y);
          acc0[v].z = fmaf(dsu, x0[u][v].z, acc0[v].z); acc0[v].w = fmaf(dsu, x0[u][v].w, acc0[v].w);
        }
        if constexpr (COL) {
          const float au = __shfl(a_l, u, L);
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            acc1[v].x = fmaf(au, x1[u][v].x, acc1[v].x); acc1[v].y = fmaf(au, x1[u][v].y, acc1[v].y);
            acc1[v].z = fmaf(au, x1[u][v].z, acc1[v].z); acc1[v].w = fmaf(au, x1[u][v].w, acc1[v].w);
          }
        }
      }
    }
  }
  if (dirty) flush(cur_row);
}

}  // namespace graphop
