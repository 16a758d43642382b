// The three gather passes of the fused GATv2 layer (kernels_gatv2_attn.h includes this file twice, inside namespace
// graphop): once with GV2_DROP = false and GV2_KERNEL(pass) = k_gv2attn_<pass>_f32, once with GV2_DROP = true and
// GV2_KERNEL(pass) = k_gv2drop_<pass>_f32.  The undropped kernels must keep their names and template argument lists, so
// DROP cannot be a template parameter of one __global__, and a shared __forceinline__ body reschedules every undropped
// kernel (DESIGN.md 4.5g); the text compiled twice leaves them instruction for instruction what they were.  `dr` is an
// empty NoDrop without dropout; only `if constexpr (DROP)` code names its members.
// GV2_EDGE (0 / 1; kernels_gatv2_edge_attn.h includes this file twice more with 1, as k_gv2edge_* and k_gv2edrop_*) adds
// the edge row: z = (xl_i + xr_j) + xe_e for edge e = eid[slot].  GV2_IF_EDGE(...) is its arguments with the edge row and
// nothing without, and `#if GV2_EDGE` picks between the two forms of z; with GV2_EDGE 0 the text is the one before the
// edge row existed.  The lanes that load a batch's neighbour ids also load its edge ids, which travel by one more
// group_bcast; a NULL eid in a row-major pass means eid[slot] == slot (a plan with eid_identity): a kernel-uniform
// branch.  xe_e is consumed where z is formed (gv2edge_z4, then gv2edge_dot4 in every pass), so no pass keeps a second
// [SB][NV] array; the row pass also stores dxe[e] = ds att t, one float4 per lane and real slot, where dxe is not NULL.
#if GV2_EDGE
#define GV2_IF_EDGE(...) __VA_ARGS__
// the edge id of the lane's slot, loaded by the lanes that load its neighbour id; eo[u] = the 64-bit row offset e * F4
#define GV2_EDGE_IDS(slot)                        \
  int my_e = 0;                                   \
  i64 eo[SB];                                     \
  if (l < IDL) {                                  \
    const i64 js = (slot);                        \
    my_e = eid ? (int)eid[js] : (int)js;          \
  }
#else
#define GV2_IF_EDGE(...)
#endif

// ---- forward -----------------------------------------------------------------------------------------------------
// Blocks [0, nb_short): lane groups of 16, one row segment each (segments above long_len slots are skipped);
// blocks nb_short + b: the whole workgroup on segment long_segs[b], its 16 groups taking batches strided and merging
// their (m, l, acc) through LDS.  xl_i and the lane's pieces of att stay in registers; a batch's SB neighbour ids are
// loaded by the first lanes and handed round by group_bcast; per batch the running maximum is raised once and
// (l, acc) rescaled once.  DROP: l sums the undropped exp(s - m), acc the terms exp(s - m) m_ijk xr_j, so stats come
// from the same expressions in the same order as without dropout.
template <int H, int D>
__global__ __launch_bounds__(kFastBlock) void GV2_KERNEL(fwd)(
    const i64* __restrict__ row, const i64* __restrict__ indptr, GV2_IF_EDGE(const i64* __restrict__ eid,)
    const i64* __restrict__ indices, const i64* __restrict__ seg_chunk, const float* __restrict__ xl,
    const float* __restrict__ xr, GV2_IF_EDGE(const float* __restrict__ xe,) const float* __restrict__ att, float* __restrict__ o, float2* __restrict__ stats, i64 n_seg, unsigned nb_short,
    i64 long_len, const int* __restrict__ long_segs, float slope, typename Gv2DropArg<H, GV2_DROP>::type dr) {
  constexpr bool DROP = GV2_DROP;
  using C = Gv2AttnCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB_FWD;
  constexpr int IDL = DROP ? GatDropCfg<H, SB>::LANES : SB;   // lanes that load a neighbour id
  constexpr i64 F4 = C::F4;
  constexpr int NG = kFastBlock / L;   // lane groups of a workgroup
  __shared__ float4 red_acc[NG][F4];
  __shared__ float2 red_ml[NG][H];
  const int l = threadIdx.x % L, g = threadIdx.x / L;
  const bool longp = blockIdx.x >= nb_short;   // workgroup-uniform
  const i64 s = longp ? (i64)long_segs[blockIdx.x - nb_short] : (i64)blockIdx.x * NG + g;
  const bool have = s < n_seg;
  i64 r = 0, j0 = 0, j1 = 0;
  if (have) {
    const i64 c0 = seg_chunk[s];
    r = row[c0];
    j0 = indptr[c0];
    j1 = indptr[seg_chunk[s + 1]];
  }
  const bool work = have && (longp || j1 - j0 <= long_len);   // group-uniform
  int kv[NV];
  float4 w[NV], a[NV], acc[NV];
  float m[NV], ls[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    kv[v] = (v * L + l) / DQ;
    acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    m[v] = kGv2AttnFloor;
    ls[v] = 0.f;
  }
  if (work) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      w[v] = ld4(att, v * L + l);
      a[v] = ld4(xl, r * F4 + v * L + l);
    }
    const i64 step = longp ? (i64)NG * SB : (i64)SB;
    for (i64 jb = longp ? j0 + (i64)g * SB : j0; jb < j1; jb += step) {
      const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
      int my_src = 0;   // slots past the end re-read the batch's last neighbour with weight 0
      const int t = DROP ? l % SB : l;
      if (l < IDL) my_src = (int)indices[jb + (t < nb ? t : nb - 1)];
      GV2_IF_EDGE(GV2_EDGE_IDS(jb + (t < nb ? t : nb - 1));)
      float4 x[SB][NV];
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        GV2_IF_EDGE(eo[u] = (i64)group_bcast<L, u>(my_e) * F4;)
#pragma unroll
        for (int v = 0; v < NV; ++v) x[u][v] = ld4(xr, src * F4 + v * L + l);
      });
      int keep[DROP ? SB : 1];
      if constexpr (DROP) {
        const int mine = gat_drop_lane_bits<H, SB, false>(l, r, my_src, dr);
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          keep[u] = gat_drop_slot_bits<H, SB, u>(mine);
        });
      }
      float sc[SB][NV];
#pragma unroll
      for (int u = 0; u < SB; ++u)
#pragma unroll
        for (int v = 0; v < NV; ++v)
#if GV2_EDGE
          sc[u][v] = group_sum<DQ>(
              gv2edge_dot4(w[v], gv2edge_z4(a[v], x[u][v], ld4_nt(xe, eo[u] + v * L + l)), slope));
#else
          sc[u][v] = group_sum<DQ>(gv2attn_dot4(w[v], a[v], x[u][v], slope));
#endif
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        float mn = m[v];
#pragma unroll
        for (int u = 0; u < SB; ++u) mn = u < nb ? fmaxf(mn, sc[u][v]) : mn;
        const float f = exp_nonpos(m[v] - mn);
        m[v] = mn;
        ls[v] *= f;
        gv2attn_scale4(acc[v], f);
#pragma unroll
        for (int u = 0; u < SB; ++u) {
          const float p = u < nb ? exp_nonpos(sc[u][v] - mn) : 0.f;
          ls[v] += p;
          if constexpr (DROP) gv2attn_fma4(acc[v], (keep[u] >> kv[v]) & 1 ? p * dr.scale : 0.f, x[u][v]);
          else gv2attn_fma4(acc[v], p, x[u][v]);
        }
      }
    }
  }
  if (!longp) {
    if (work) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const float il = ls[v] > 0.f ? 1.f / ls[v] : 0.f;
        gv2attn_scale4(acc[v], il);
        reinterpret_cast<float4*>(o)[r * F4 + v * L + l] = acc[v];
        if (l % DQ == 0) stats[r * H + kv[v]] = make_float2(m[v], il);
      }
    }
    return;
  }
  // long segment (workgroup-uniform branch): every group publishes (m, l) per head and acc per piece (16 KB + 1 KB of
  // LDS at h * d = 256); thread p < F4 merges piece p
  // over the groups in a fixed order
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    red_acc[g][v * L + l] = acc[v];
    if (l % DQ == 0) red_ml[g][kv[v]] = make_float2(m[v], ls[v]);
  }
  __syncthreads();
  if (have && threadIdx.x < F4) {
    const int p = threadIdx.x, k = p / DQ;
    float mm = kGv2AttnFloor;
#pragma unroll
    for (int q = 0; q < NG; ++q) mm = fmaxf(mm, red_ml[q][k].x);
    float lsum = 0.f;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int q = 0; q < NG; ++q) {
      const float2 ml = red_ml[q][k];
      const float f = exp_nonpos(ml.x - mm);
      lsum = fmaf(ml.y, f, lsum);
      gv2attn_fma4(t, f, red_acc[q][p]);
    }
    const float il = lsum > 0.f ? 1.f / lsum : 0.f;
    gv2attn_scale4(t, il);
    reinterpret_cast<float4*>(o)[r * F4 + p] = t;
    if (p % DQ == 0) stats[r * H + k] = make_float2(mm, il);
  }
}

// ---- backward passes -------------------------------------------------------------------------------------------------
// The chunk driver: a lane group takes chunks_per_group adjacent chunks and keeps the own node's rows in registers
// while the node does not change; sums leave once per (lane group, node): stored where the group owns the node
// (OWNED: sorted chunk list and the neighbouring groups' chunks name other nodes), added by float atomics otherwise.

// row pass: own = xl_i, dO_i, P[i]; gathered = xr_j.  The row sum is kept as sum_j ds t and multiplied by att when the
// row leaves.  The lane's pieces of datt are summed over the group's whole run, reduced over the workgroup (shuffles
// inside a wave, LDS across waves) and written as row blockIdx.x of datt_part (gridDim.x, F4): every workgroup writes
// its row, groups without chunks add zeros.  DROP: da_ij = m_ij <dO_i, xr_j>; D_i in P is <dO_i, o_i> of the dropped o.
template <int H, int D, bool OWNED>
__global__ __launch_bounds__(kFastBlock) void GV2_KERNEL(bwd_row)(
    const i64* __restrict__ row, const i64* __restrict__ indptr, GV2_IF_EDGE(const i64* __restrict__ eid,)
    const i64* __restrict__ indices, const float* __restrict__ xl, const float* __restrict__ xr,
    GV2_IF_EDGE(const float* __restrict__ xe,) const float* __restrict__ att, const float4* __restrict__ P,
    const float* __restrict__ dO, float* __restrict__ dxl, GV2_IF_EDGE(float* __restrict__ dxe,)
    float4* __restrict__ datt_part, i64 n_chunks, int chunks_per_group, float slope,
    typename Gv2DropArg<H, GV2_DROP>::type dr) {
  constexpr bool DROP = GV2_DROP;
  using C = Gv2AttnCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB_ROW;
  constexpr int IDL = DROP ? GatDropCfg<H, SB>::LANES : SB;   // lanes that load a neighbour id
  constexpr i64 F4 = C::F4;
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  int kv[NV];
  float4 w[NV], a[NV], g[NV], acc[NV], dw[NV];
  float pm[NV], pil[NV], pd[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    kv[v] = (v * L + l) / DQ;
    w[v] = ld4(att, v * L + l);
    acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    dw[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (c0 < c1) {   // group-uniform
    i64 row_before = -1, row_after = -1;
    if constexpr (OWNED) {
      if (c0 > 0) row_before = row[c0 - 1];
      if (c1 < n_chunks) row_after = row[c1];
    }
    auto flush = [&](i64 r) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        acc[v].x *= w[v].x; acc[v].y *= w[v].y; acc[v].z *= w[v].z; acc[v].w *= w[v].w;
      }
      if (OWNED && r != row_before && r != row_after) {
#pragma unroll
        for (int v = 0; v < NV; ++v) reinterpret_cast<float4*>(dxl)[r * F4 + v * L + l] = acc[v];
      } else {
        atomic_flush<L, NV>(dxl, r, acc, l);
      }
#pragma unroll
      for (int v = 0; v < NV; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    };
    i64 cur = -1;
    bool dirty = false;
    for (i64 c = c0; c < c1; ++c) {
      const i64 r = row[c];
      if (r != cur) {
        if (dirty) { flush(cur); dirty = false; }
        cur = r;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          a[v] = ld4(xl, r * F4 + v * L + l);
          g[v] = ld4(dO, r * F4 + v * L + l);
          const float4 p = P[r * H + kv[v]];
          pm[v] = p.x; pil[v] = p.y; pd[v] = p.z;
        }
      }
      const i64 j0 = indptr[c], j1 = indptr[c + 1];
      if (j1 > j0) dirty = true;
      for (i64 jb = j0; jb < j1; jb += SB) {
        const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
        int my_src = 0;   // slots past the end re-read the batch's last neighbour with weight 0
        const int t = DROP ? l % SB : l;
        if (l < IDL) my_src = (int)indices[jb + (t < nb ? t : nb - 1)];
        GV2_IF_EDGE(GV2_EDGE_IDS(jb + (t < nb ? t : nb - 1));)
        float4 x[SB][NV];
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          const i64 src = group_bcast<L, u>(my_src);
          GV2_IF_EDGE(eo[u] = (i64)group_bcast<L, u>(my_e) * F4;)
#pragma unroll
          for (int v = 0; v < NV; ++v) x[u][v] = ld4(xr, src * F4 + v * L + l);
        });
        int keep[DROP ? SB : 1];
        if constexpr (DROP) {
          const int mine = gat_drop_lane_bits<H, SB, false>(l, r, my_src, dr);
          static_for<SB>([&](auto uc) {
            constexpr int u = decltype(uc)::value;
            keep[u] = gat_drop_slot_bits<H, SB, u>(mine);
          });
        }
#pragma unroll
        for (int u = 0; u < SB; ++u) {
#pragma unroll
          for (int v = 0; v < NV; ++v) {
#if GV2_EDGE
            const float4 z = gv2edge_z4(a[v], x[u][v], ld4_nt(xe, eo[u] + v * L + l));
            float s = gv2edge_dot4(w[v], z, slope), da = dot4(g[v], x[u][v]);   // x[u][v] is dead from here: z lives on
#else
            float s = gv2attn_dot4(w[v], a[v], x[u][v], slope), da = dot4(g[v], x[u][v]);
#endif
            gv2attn_group_sum2<DQ>(s, da);
            if constexpr (DROP) da = (keep[u] >> kv[v]) & 1 ? da * dr.scale : 0.f;
            const float aij = u < nb ? exp_nonpos(s - pm[v]) * pil[v] : 0.f;
            const float ds = aij * (da - pd[v]), dss = ds * slope;
#if GV2_EDGE
            const float zx = z.x, zy = z.y, zz = z.z, zw = z.w;
            if (dxe != nullptr && u < nb)   // the row-major orientation visits a slot once: a plain store
              reinterpret_cast<float4*>(dxe)[eo[u] + v * L + l] =
                  make_float4((zx > 0.f ? ds : dss) * w[v].x, (zy > 0.f ? ds : dss) * w[v].y,
                              (zz > 0.f ? ds : dss) * w[v].z, (zw > 0.f ? ds : dss) * w[v].w);
#else
            const float zx = a[v].x + x[u][v].x, zy = a[v].y + x[u][v].y;
            const float zz = a[v].z + x[u][v].z, zw = a[v].w + x[u][v].w;
#endif
            acc[v].x += zx > 0.f ? ds : dss;
            acc[v].y += zy > 0.f ? ds : dss;
            acc[v].z += zz > 0.f ? ds : dss;
            acc[v].w += zw > 0.f ? ds : dss;
            dw[v].x = fmaf(ds, gv2attn_lrelu(zx, slope), dw[v].x);
            dw[v].y = fmaf(ds, gv2attn_lrelu(zy, slope), dw[v].y);
            dw[v].z = fmaf(ds, gv2attn_lrelu(zz, slope), dw[v].z);
            dw[v].w = fmaf(ds, gv2attn_lrelu(zw, slope), dw[v].w);
          }
        }
      }
    }
    if (dirty) flush(cur);
  }
  // every thread of the workgroup arrives here
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

// column pass: own = xr_j; gathered = xl_i, dO_i and P[i]; dxr[j] += sum_i (ds att t + a dO_i).  DROP: the decision's
// counter stays (i, j) = (gathered id, own column); da_ij = m_ij <dO_i, xr_j> and the second term is a_ij m_ij dO_i.
template <int H, int D, bool OWNED>
__global__ __launch_bounds__(kFastBlock) void GV2_KERNEL(bwd_col)(
    const i64* __restrict__ col, const i64* __restrict__ indptr, GV2_IF_EDGE(const i64* __restrict__ eid,)
    const i64* __restrict__ indices, const float* __restrict__ xl, const float* __restrict__ xr,
    GV2_IF_EDGE(const float* __restrict__ xe,) const float* __restrict__ att, const float4* __restrict__ P,
    const float* __restrict__ dO, float* __restrict__ dxr, i64 n_chunks,
    int chunks_per_group, float slope, typename Gv2DropArg<H, GV2_DROP>::type dr) {
  constexpr bool DROP = GV2_DROP;
  using C = Gv2AttnCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB_COL;
  constexpr int IDL = DROP ? GatDropCfg<H, SB>::LANES : SB;   // lanes that load a neighbour id
  constexpr i64 F4 = C::F4;
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  if (c0 >= c1) return;
  i64 col_before = -1, col_after = -1;
  if constexpr (OWNED) {
    if (c0 > 0) col_before = col[c0 - 1];
    if (c1 < n_chunks) col_after = col[c1];
  }
  int kv[NV];
  float4 w[NV], b[NV], acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    kv[v] = (v * L + l) / DQ;
    w[v] = ld4(att, v * L + l);
    acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  auto flush = [&](i64 r) {
    if (OWNED && r != col_before && r != col_after) {
#pragma unroll
      for (int v = 0; v < NV; ++v) reinterpret_cast<float4*>(dxr)[r * F4 + v * L + l] = acc[v];
    } else {
      atomic_flush<L, NV>(dxr, r, acc, l);
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  };
  i64 cur = -1;
  bool dirty = false;
  for (i64 c = c0; c < c1; ++c) {
    const i64 r = col[c];
    if (r != cur) {
      if (dirty) { flush(cur); dirty = false; }
      cur = r;
#pragma unroll
      for (int v = 0; v < NV; ++v) b[v] = ld4(xr, r * F4 + v * L + l);
    }
    const i64 j0 = indptr[c], j1 = indptr[c + 1];
    if (j1 > j0) dirty = true;
    for (i64 jb = j0; jb < j1; jb += SB) {
      const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
      int my_src = 0;   // slots past the end re-read the batch's last neighbour with weight 0
      const int t = DROP ? l % SB : l;
      if (l < IDL) my_src = (int)indices[jb + (t < nb ? t : nb - 1)];
      GV2_IF_EDGE(GV2_EDGE_IDS(jb + (t < nb ? t : nb - 1));)
      float4 x[SB][NV], y[SB][NV], p[SB][NV];   // xl_i, dO_i, P[i, k_v]
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        GV2_IF_EDGE(eo[u] = (i64)group_bcast<L, u>(my_e) * F4;)
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          x[u][v] = ld4(xl, src * F4 + v * L + l);
          y[u][v] = ld4(dO, src * F4 + v * L + l);
          p[u][v] = P[src * H + kv[v]];
        }
      });
      int keep[DROP ? SB : 1];
      if constexpr (DROP) {
        const int mine = gat_drop_lane_bits<H, SB, true>(l, r, my_src, dr);
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          keep[u] = gat_drop_slot_bits<H, SB, u>(mine);
        });
      }
#pragma unroll
      for (int u = 0; u < SB; ++u) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
#if GV2_EDGE
          const float4 z = gv2edge_z4(x[u][v], b[v], ld4(xe, eo[u] + v * L + l));   // a random row read: e = eid_c[slot]
          float s = gv2edge_dot4(w[v], z, slope), da = dot4(y[u][v], b[v]);
#else
          float s = gv2attn_dot4(w[v], x[u][v], b[v], slope), da = dot4(y[u][v], b[v]);
#endif
          gv2attn_group_sum2<DQ>(s, da);
          const float aij = u < nb ? exp_nonpos(s - p[u][v].x) * p[u][v].y : 0.f;
          float am = aij;   // a_ij m_ij
          if constexpr (DROP) {
            const float m = (keep[u] >> kv[v]) & 1 ? dr.scale : 0.f;
            da *= m;
            am *= m;
          }
          const float ds = aij * (da - p[u][v].z), dss = ds * slope;
#if GV2_EDGE
          const float zx = z.x, zy = z.y, zz = z.z, zw = z.w;
#else
          const float zx = x[u][v].x + b[v].x, zy = x[u][v].y + b[v].y;
          const float zz = x[u][v].z + b[v].z, zw = x[u][v].w + b[v].w;
#endif
          acc[v].x = fmaf(zx > 0.f ? ds : dss, w[v].x, fmaf(am, y[u][v].x, acc[v].x));
          acc[v].y = fmaf(zy > 0.f ? ds : dss, w[v].y, fmaf(am, y[u][v].y, acc[v].y));
          acc[v].z = fmaf(zz > 0.f ? ds : dss, w[v].z, fmaf(am, y[u][v].z, acc[v].z));
          acc[v].w = fmaf(zw > 0.f ? ds : dss, w[v].w, fmaf(am, y[u][v].w, acc[v].w));
        }
      }
    }
  }
  if (dirty) flush(cur);
}

#undef GV2_IF_EDGE
#if GV2_EDGE
#undef GV2_EDGE_IDS
#endif
