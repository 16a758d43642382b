// The gather passes of the fused GAT layer, with and without an edge term in the score.  Included twice, inside
// namespace graphop:
//   kernels_gat_attn.h       GA_EDGE 0   z = el[i] + er[j]             k_gat_attn_*,      gat_attn_bwd_walk / _dz
//   kernels_gat_edge_attn.h  GA_EDGE 1   z = (el[i] + er[j]) + ee[e]   k_gat_edge_attn_*, gat_edge_attn_bwd_walk / _dz
// The includer defines GA_EDGE, GA_KERNEL(pass, kind) and GA_FN(name), and undefines them afterwards.  GA_IF_EDGE(...)
// is its arguments with the edge term and nothing without: the eid / ee / dee parameters, the loads of a slot's edge id
// and its h values of ee, the `+ ee` of the score and the dee store.  Expanding to nothing (rather than a template
// argument or an `if constexpr`) keeps the plain kernels' names, template argument lists and parameter lists, so their
// kernarg layout, what they were; and a shared __forceinline__ body with a `bool EDGE` reschedules the fast kernels of
// both ops (DESIGN.md 4.5h), while the text compiled twice leaves every kernel instruction for instruction what it was.
// A NULL eid in a fast kernel means eid[slot] == slot (a plan with eid_identity): a kernel-uniform branch.
#if GA_EDGE
#define GA_IF_EDGE(...) __VA_ARGS__
#else
#define GA_IF_EDGE(...)
#endif

// ---- stats pass --------------------------------------------------------------------------------------------------
// Blocks [0, nb_short): lane groups of G lanes, one row segment each (segments above long_len slots are skipped);
// blocks nb_short + b: the whole workgroup on segment long_segs[b].  Every lane keeps an online (m, l) per head over
// its slots; the group merges them by butterfly (and the workgroup through LDS).
template <int H, int G>
__global__ __launch_bounds__(kFastBlock) void GA_KERNEL(stats, f32)(
    const i64* __restrict__ row, const i64* __restrict__ indptr, GA_IF_EDGE(const i64* __restrict__ eid,)
    const i64* __restrict__ indices, const i64* __restrict__ seg_chunk, const float* __restrict__ el,
    const float* __restrict__ er, GA_IF_EDGE(const float* __restrict__ ee,) float2* __restrict__ stats, i64 n_seg,
    unsigned nb_short, i64 long_len, const int* __restrict__ long_segs, float slope) {
  constexpr int W = H >= 4 ? 4 : H;
  constexpr int NI = H / W;   // items of er (and ee) per slot
  __shared__ float red[2][kFastBlock / kWave][H];
  const bool longp = blockIdx.x >= nb_short;
  int gl, gw;       // lane and width of the reducing group
  i64 s;
  if (longp) {
    s = long_segs[blockIdx.x - nb_short];
    gl = threadIdx.x;
    gw = kFastBlock;
  } else {
    s = (i64)blockIdx.x * (kFastBlock / G) + threadIdx.x / G;
    gl = threadIdx.x % G;
    gw = G;
  }
  const bool have = s < n_seg;
  i64 r = 0, j0 = 0, j1 = 0;
  if (have) {
    const i64 c0 = seg_chunk[s];
    r = row[c0];
    j0 = indptr[c0];
    j1 = indptr[seg_chunk[s + 1]];
  }
  const bool work = have && (longp || j1 - j0 <= long_len);
  float a[H], m[H], l[H];
  if (work) {
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      const GatItem<W> t = gat_ld<W>(el + r * H + k * W);
#pragma unroll
      for (int i = 0; i < W; ++i) a[k * W + i] = t.v[i];
    }
  }
#pragma unroll
  for (int k = 0; k < H; ++k) { m[k] = kGatAttnFloor; l[k] = 0.f; }
  if (work) {
    i64 j = j0 + gl;
    for (; j + gw < j1; j += 2 * gw) {   // two independent gathers in flight
      const i64 s0 = indices[j], s1 = indices[j + gw];
      GA_IF_EDGE(const i64 e0 = eid ? eid[j] : j, e1 = eid ? eid[j + gw] : j + gw;)
      GatItem<W> b0[NI], b1[NI] GA_IF_EDGE(, g0[NI], g1[NI]);
#pragma unroll
      for (int k = 0; k < NI; ++k) {
        b0[k] = gat_ld<W>(er + s0 * H + k * W); b1[k] = gat_ld<W>(er + s1 * H + k * W);
        GA_IF_EDGE(g0[k] = gat_ld<W>(ee + e0 * H + k * W); g1[k] = gat_ld<W>(ee + e1 * H + k * W);)
      }
#pragma unroll
      for (int k = 0; k < NI; ++k)
#pragma unroll
        for (int i = 0; i < W; ++i) {
          const int hh = k * W + i;
          const float z0 = gat_lrelu((a[hh] + b0[k].v[i]) GA_IF_EDGE(+ g0[k].v[i]), slope);
          const float z1 = gat_lrelu((a[hh] + b1[k].v[i]) GA_IF_EDGE(+ g1[k].v[i]), slope);
          const float mx = fmaxf(z0, z1);
          gat_attn_merge(m[hh], l[hh], mx, exp_nonpos(z0 - mx) + exp_nonpos(z1 - mx));
        }
    }
    if (j < j1) {
      const i64 s0 = indices[j];
      GA_IF_EDGE(const i64 e0 = eid ? eid[j] : j;)
#pragma unroll
      for (int k = 0; k < NI; ++k) {
        const GatItem<W> b0 = gat_ld<W>(er + s0 * H + k * W);
        GA_IF_EDGE(const GatItem<W> g0 = gat_ld<W>(ee + e0 * H + k * W);)
#pragma unroll
        for (int i = 0; i < W; ++i) {
          const int hh = k * W + i;
          gat_attn_merge(m[hh], l[hh], gat_lrelu((a[hh] + b0.v[i]) GA_IF_EDGE(+ g0.v[i]), slope), 1.f);
        }
      }
    }
  }
  // butterfly over the group's lanes (a wave at most)
  const int wl = gw < kWave ? gw : kWave;
#pragma unroll
  for (int k = 0; k < H; ++k)
    for (int o = 1; o < wl; o <<= 1) gat_attn_merge(m[k], l[k], __shfl_xor(m[k], o), __shfl_xor(l[k], o));
  if (longp) {   // workgroup-uniform branch: the waves' results through LDS
    const int w = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
      for (int k = 0; k < H; ++k) { red[0][w][k] = m[k]; red[1][w][k] = l[k]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < H; ++k)
        for (int q = 1; q < kFastBlock / kWave; ++q) gat_attn_merge(m[k], l[k], red[0][q][k], red[1][q][k]);
    }
  }
  if (work && gl == 0) {
#pragma unroll
    for (int k = 0; k < H; ++k) stats[r * H + k] = make_float2(m[k], l[k] > 0.f ? 1.f / l[k] : 0.f);
  }
}

// ---- forward aggregation ---------------------------------------------------------------------------------------
// Chunk driver: el_i, (m_i, 1/l_i) and the output row stay in registers while the row is unchanged.  The lanes that
// load a batch's neighbour ids also load its edge ids; per slot er_j and V_j (and ee_e) are gathered.
// DROP: the weight of a slot is multiplied by m_ijk (the row statistics are those of the undropped scores).
template <int H, int D, bool OWNED, bool DROP>
__global__ __launch_bounds__(kFastBlock) void GA_KERNEL(fwd, f32)(
    const i64* __restrict__ row, const i64* __restrict__ indptr, GA_IF_EDGE(const i64* __restrict__ eid,)
    const i64* __restrict__ indices, const float* __restrict__ el, const float* __restrict__ er,
    GA_IF_EDGE(const float* __restrict__ ee,) const float2* __restrict__ stats, const float* __restrict__ V,
    float* __restrict__ o, i64 n_chunks, int chunks_per_group, float slope, DropArgsIf<DROP, float> dr) {
  using C = GatAttnCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, SB = C::SB_FWD;
  constexpr int IDL = DROP ? GatDropCfg<H, SB>::LANES : SB;   // lanes that load a neighbour id
  constexpr i64 F4 = C::F4;
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  if (c0 >= c1) return;
  i64 row_before = -1, row_after = -1;
  if constexpr (OWNED) {
    if (c0 > 0) row_before = row[c0 - 1];
    if (c1 < n_chunks) row_after = row[c1];
  }
  int kv[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) kv[v] = gat_attn_head<H, D>(v, l);
  float4 acc[NV];
  float a_el[NV], a_m[NV], a_il[NV];
  auto zero_acc = [&]() {
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto flush = [&](i64 r) {
    if (OWNED && r != row_before && r != row_after) {
#pragma unroll
      for (int v = 0; v < NV; ++v) reinterpret_cast<float4*>(o)[r * F4 + v * L + l] = acc[v];
    } else {
      atomic_flush<L, NV>(o, r, acc, l);
    }
  };
  zero_acc();
  i64 cur = -1;
  bool dirty = false;
  for (i64 c = c0; c < c1; ++c) {
    const i64 r = row[c];
    if (r != cur) {
      if (dirty) { flush(cur); zero_acc(); dirty = false; }
      cur = r;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        a_el[v] = el[r * H + kv[v]];
        const float2 st = stats[r * H + kv[v]];
        a_m[v] = st.x;
        a_il[v] = st.y;
      }
    }
    const i64 j0 = indptr[c], j1 = indptr[c + 1];
    if (j1 > j0) dirty = true;
    for (i64 jb = j0; jb < j1; jb += SB) {
      const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
      int my_src = 0 GA_IF_EDGE(, my_e = 0);   // slots past the end re-read the batch's last slot with weight 0
      const int t = DROP ? l % SB : l;
      if (l < IDL) {
        const i64 j = jb + (t < nb ? t : nb - 1);
        my_src = (int)indices[j];
        GA_IF_EDGE(my_e = eid ? (int)eid[j] : (int)j;)
      }
      float4 x[SB][NV];
      float e[SB][NV] GA_IF_EDGE(, g[SB][NV]);
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        GA_IF_EDGE(const i64 ed = group_bcast<L, u>(my_e);)
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          x[u][v] = reinterpret_cast<const float4*>(V)[src * F4 + v * L + l];
          e[u][v] = er[src * H + kv[v]];
          GA_IF_EDGE(g[u][v] = ee[ed * H + kv[v]];)
        }
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
          const float z = gat_lrelu((a_el[v] + e[u][v]) GA_IF_EDGE(+ g[u][v]), slope);
          float w = u < nb ? exp_nonpos(z - a_m[v]) * a_il[v] : 0.f;
          if constexpr (DROP) w = (keep[u] >> kv[v]) & 1 ? w * dr.scale : 0.f;
          acc[v].x = fmaf(w, x[u][v].x, acc[v].x); acc[v].y = fmaf(w, x[u][v].y, acc[v].y);
          acc[v].z = fmaf(w, x[u][v].z, acc[v].z); acc[v].w = fmaf(w, x[u][v].w, acc[v].w);
        }
      }
    }
  }
  if (dirty) flush(cur);
}

// ---- backward passes -----------------------------------------------------------------------------------------------
// ROW (row-major chunks): own = dO_i and P[i] in registers; gathers er_j and V_j (and ee_e); out0 = del, and
//   dee[e] = dz_e where dee is not NULL: the head's first lane stores it, for the batch's real slots only.
// COL (column-major chunks): own = V_j and er_j in registers; gathers P[i] and dO_i (and ee_e, e = eid_c[slot]: a random
//   4-byte read per slot and head, inherent while nothing edge-sized may be staged); out0 = der, out1 = dV.
// DROP: da_ij = m_ij <dO_i, V_j> and dV_j sums a_ij m_ij dO_i; D_i in P is <dO_i, o_i> of the dropped o.
template <int H, int D, bool COL, bool OWNED, bool DROP>
__device__ __forceinline__ void GA_FN(bwd_walk)(
    const i64* __restrict__ seg, const i64* __restrict__ indptr, GA_IF_EDGE(const i64* __restrict__ eid,)
    const i64* __restrict__ indices, const float* __restrict__ er, GA_IF_EDGE(const float* __restrict__ ee,)
    const float* __restrict__ V, const float4* __restrict__ P, const float* __restrict__ dO,
    float* __restrict__ out0, float* __restrict__ out1, GA_IF_EDGE(float* __restrict__ dee,) i64 n_chunks,
    int chunks_per_group, float slope, const DropArgsIf<DROP, float>& dr) {
  using C = GatAttnCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB_BWD;
  constexpr int IDL = DROP ? GatDropCfg<H, SB>::LANES : SB;   // lanes that load a neighbour id
  constexpr i64 F4 = C::F4;
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  if (c0 >= c1) return;
  i64 row_before = -1, row_after = -1;
  if constexpr (OWNED) {
    if (c0 > 0) row_before = seg[c0 - 1];
    if (c1 < n_chunks) row_after = seg[c1];
  }
  int kv[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) kv[v] = gat_attn_head<H, D>(v, l);
  float4 y[NV];              // ROW: dO_i   COL: V_j
  float4 p_own[NV];          // ROW: P[i, k_v]
  float e_own[NV];           // COL: er[j, k_v]
  float acc[NV];             // dz sums of the piece's head
  float4 accv[COL ? NV : 1]; // COL: dV_j
  auto zero_acc = [&]() {
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.f;
#pragma unroll
    for (int v = 0; v < (COL ? NV : 1); ++v) accv[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto flush = [&](i64 r) {
    const bool own = OWNED && r != row_before && r != row_after;
    if (l % DQ == 0) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        if (own) out0[r * H + kv[v]] = acc[v];
        else atomicAdd(out0 + r * H + kv[v], acc[v]);
      }
    }
    if constexpr (COL) {
      if (own) {
#pragma unroll
        for (int v = 0; v < NV; ++v) reinterpret_cast<float4*>(out1)[r * F4 + v * L + l] = accv[v];
      } else {
        atomic_flush<L, NV>(out1, r, accv, l);
      }
    }
  };
  zero_acc();
  i64 cur = -1;
  bool dirty = false;
  for (i64 c = c0; c < c1; ++c) {
    const i64 r = seg[c];
    if (r != cur) {
      if (dirty) { flush(cur); zero_acc(); dirty = false; }
      cur = r;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        y[v] = reinterpret_cast<const float4*>(COL ? V : dO)[r * F4 + v * L + l];
        if constexpr (COL) e_own[v] = er[r * H + kv[v]];
        else p_own[v] = P[r * H + kv[v]];
      }
    }
    const i64 j0 = indptr[c], j1 = indptr[c + 1];
    if (j1 > j0) dirty = true;
    for (i64 jb = j0; jb < j1; jb += SB) {
      const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
      int my_src = 0 GA_IF_EDGE(, my_e = 0);
      const int t = DROP ? l % SB : l;
      if (l < IDL) {
        const i64 j = jb + (t < nb ? t : nb - 1);
        my_src = (int)indices[j];
        GA_IF_EDGE(my_e = eid ? (int)eid[j] : (int)j;)
      }
      float4 x[SB][NV];        // ROW: V_j   COL: dO_i
      float4 pg[COL ? SB : 1][NV];
      float eg[COL ? 1 : SB][NV];
      GA_IF_EDGE(float g[SB][NV]; int ed[SB];)   // ee_e and e
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        GA_IF_EDGE(ed[u] = group_bcast<L, u>(my_e);)
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          x[u][v] = reinterpret_cast<const float4*>(COL ? dO : V)[src * F4 + v * L + l];
          if constexpr (COL) pg[u][v] = P[src * H + kv[v]];
          else eg[u][v] = er[src * H + kv[v]];
          GA_IF_EDGE(g[u][v] = ee[(i64)ed[u] * H + kv[v]];)
        }
      });
      int keep[DROP ? SB : 1];
      if constexpr (DROP) {
        const int mine = gat_drop_lane_bits<H, SB, COL>(l, r, my_src, dr);
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          keep[u] = gat_drop_slot_bits<H, SB, u>(mine);
        });
      }
#pragma unroll
      for (int u = 0; u < SB; ++u) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          float da = group_sum<DQ>(dot4(y[v], x[u][v]));
          float4 p;
          float z;
          if constexpr (COL) { p = pg[u][v]; z = (p.x + e_own[v]) GA_IF_EDGE(+ g[u][v]); }
          else { p = p_own[v]; z = (p.x + eg[u][v]) GA_IF_EDGE(+ g[u][v]); }
          const float a = u < nb ? exp_nonpos(gat_lrelu(z, slope) - p.y) * p.z : 0.f;
          float am = a;   // a_ij m_ij
          if constexpr (DROP) {
            const float m = (keep[u] >> kv[v]) & 1 ? dr.scale : 0.f;
            da *= m;
            am *= m;
          }
          const float ds = a * (da - p.w);
          const float dz = z > 0.f ? ds : ds * slope;
          acc[v] += dz;
          if constexpr (COL) {
            accv[v].x = fmaf(am, x[u][v].x, accv[v].x); accv[v].y = fmaf(am, x[u][v].y, accv[v].y);
            accv[v].z = fmaf(am, x[u][v].z, accv[v].z); accv[v].w = fmaf(am, x[u][v].w, accv[v].w);
          }
          GA_IF_EDGE(else { if (dee && u < nb && l % DQ == 0) dee[(i64)ed[u] * H + kv[v]] = dz; })
        }
      }
    }
  }
  if (dirty) flush(cur);
}

template <int H, int D, bool OWNED, bool DROP>
__global__ __launch_bounds__(kFastBlock) void GA_KERNEL(bwd_row, f32)(
    const i64* __restrict__ row, const i64* __restrict__ indptr, GA_IF_EDGE(const i64* __restrict__ eid,)
    const i64* __restrict__ indices, const float* __restrict__ er, GA_IF_EDGE(const float* __restrict__ ee,)
    const float* __restrict__ V, const float4* __restrict__ P, const float* __restrict__ dO, float* __restrict__ del,
    GA_IF_EDGE(float* __restrict__ dee,) i64 n_chunks, int chunks_per_group, float slope, DropArgsIf<DROP, float> dr) {
  GA_FN(bwd_walk)<H, D, false, OWNED, DROP>(row, indptr, GA_IF_EDGE(eid,) indices, er, GA_IF_EDGE(ee,) V, P, dO, del,
                                            nullptr, GA_IF_EDGE(dee,) n_chunks, chunks_per_group, slope, dr);
}

template <int H, int D, bool OWNED, bool DROP>
__global__ __launch_bounds__(kFastBlock) void GA_KERNEL(bwd_col, f32)(
    const i64* __restrict__ col, const i64* __restrict__ indptr, GA_IF_EDGE(const i64* __restrict__ eid,)
    const i64* __restrict__ indices, const float* __restrict__ er, GA_IF_EDGE(const float* __restrict__ ee,)
    const float* __restrict__ V, const float4* __restrict__ P, const float* __restrict__ dO, float* __restrict__ der,
    float* __restrict__ dV, i64 n_chunks, int chunks_per_group, float slope, DropArgsIf<DROP, float> dr) {
  GA_FN(bwd_walk)<H, D, true, OWNED, DROP>(col, indptr, GA_IF_EDGE(eid,) indices, er, GA_IF_EDGE(ee,) V, P, dO, der,
                                           dV, GA_IF_EDGE(nullptr,) n_chunks, chunks_per_group, slope, dr);
}

// ---- generic kernels: fp32 / fp64, any h and d, any chunk layout; one wave per chunk -----------------------------
// stats (n_l, h, 2) doubles as scratch: k_gat_attn_stats_init_generic fills it with (-1e9, 0), the kernel below adds
// the maximum (SUM = false) and then the sum of exp(s - m) (SUM = true) by atomics, k_gat_attn_stats_fin_generic
// leaves 1 / sum.  Lanes are (slot, head) pairs when h divides the wave (hp = h heads at a time), else one head at a
// time.  The wave walks the chunks [c, c1): without the edge term its own chunk, one atomic per (chunk, head); with it
// the run of consecutive chunks of a row that starts at its chunk, one atomic per (run, head).  A row whose chunks are
// consecutive (any sorted chunk list) is then summed in a fixed order, and its statistics are the same bit for bit
// from launch to launch; only a row scattered over several runs is added in arrival order.
template <typename T, bool SUM>
__global__ __launch_bounds__(kGenericBlock) void GA_KERNEL(stats, generic)(
    const i64* __restrict__ row, const i64* __restrict__ indptr, GA_IF_EDGE(const i64* __restrict__ eid,)
    const i64* __restrict__ indices, const T* __restrict__ el, const T* __restrict__ er,
    GA_IF_EDGE(const T* __restrict__ ee,) T* __restrict__ stats, i64 n_chunks, i64 h, T slope) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = row[c];
  constexpr bool RUNS = GA_EDGE;
  i64 c1 = c + 1;
  if constexpr (RUNS) {
    if (c > 0 && row[c - 1] == r) return;   // wave-uniform: the run belongs to the wave of its first chunk
    while (c1 < n_chunks && row[c1] == r) ++c1;
  } else {
    const i64 j0 = indptr[c], j1 = indptr[c1];
    if (j1 <= j0) return;   // wave-uniform
  }
  const int hp = (h <= kWave && kWave % h == 0) ? (int)h : 1;
  const int spw = kWave / hp;
  for (i64 kb = 0; kb < h; kb += hp) {
    const i64 k = kb + lane % hp;
    const T a = el[r * h + k];
    const T m = SUM ? stats[(r * h + k) * 2] : (T)0;
    T acc = SUM ? (T)0 : (T)-1e9;
    for (i64 cc = c; cc < c1; ++cc) {
      const i64 j1 = indptr[cc + 1];
      for (i64 j = indptr[cc] + lane / hp; j < j1; j += spw) {
        const T z = gat_lrelu((a + er[indices[j] * h + k]) GA_IF_EDGE(+ ee[eid[j] * h + k]), slope);
        if constexpr (SUM) acc += exp_t(z - m);
        else acc = z > acc ? z : acc;
      }
      if constexpr (!RUNS) break;   // c1 == c + 1, said so that no loop is left for the optimiser to remove
    }
    for (int o = hp; o < kWave; o <<= 1) {
      const T t = __shfl_xor(acc, o);
      if constexpr (SUM) acc += t;
      else acc = t > acc ? t : acc;
    }
    if (lane < hp) {
      if constexpr (SUM) atomicAdd(stats + (r * h + k) * 2 + 1, acc);
      else atomic_max_float(stats + (r * h + k) * 2, acc);
    }
  }
}

template <typename T, bool DROP>
__global__ __launch_bounds__(kGenericBlock) void GA_KERNEL(fwd, generic)(
    const i64* __restrict__ row, const i64* __restrict__ indptr, GA_IF_EDGE(const i64* __restrict__ eid,)
    const i64* __restrict__ indices, const T* __restrict__ el, const T* __restrict__ er,
    GA_IF_EDGE(const T* __restrict__ ee,) const T* __restrict__ stats, const T* __restrict__ V, T* __restrict__ o,
    i64 n_chunks, i64 h, i64 d, T slope, DropArgsIf<DROP, T> dr) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = row[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  if (j1 <= j0) return;
  for (i64 it = lane; it < h * d; it += kWave) {
    const i64 k = it / d;
    const T a = el[r * h + k], m = stats[(r * h + k) * 2], il = stats[(r * h + k) * 2 + 1];
    T acc = 0;
    for (i64 j = j0; j < j1; ++j) {
      const i64 src = indices[j];
      T w = exp_t(gat_lrelu((a + er[src * h + k]) GA_IF_EDGE(+ ee[eid[j] * h + k]), slope) - m) * il;
      if constexpr (DROP) w *= drop_mult<T>(r, src, k, dr);
      acc += w * V[src * h * d + it];
    }
    atomicAdd(o + r * h * d + it, acc);
  }
}

// dz of one slot: i = the row-major row (P[i] holds el, m, 1/l, D), j = the column, e = the edge; g = dO_i, x = V_j
// (head k slices); mult = the slot's dropout multiplier m_ij (1 without dropout)
template <typename T>
__device__ __forceinline__ T GA_FN(dz)(const T* __restrict__ p, T erj, GA_IF_EDGE(T eej,) const T* __restrict__ g,
                                       const T* __restrict__ x, i64 d, T slope, T mult) {
  const T z = (p[0] + erj) GA_IF_EDGE(+ eej);
  const T a = exp_t(gat_lrelu(z, slope) - p[1]) * p[2];
  T da = 0;
  for (i64 t = 0; t < d; ++t) da += g[t] * x[t];
  const T ds = a * (mult * da - p[3]);
  return z > (T)0 ? ds : ds * slope;
}

template <typename T, bool DROP>
__global__ __launch_bounds__(kGenericBlock) void GA_KERNEL(bwd_row, generic)(
    const i64* __restrict__ row, const i64* __restrict__ indptr, GA_IF_EDGE(const i64* __restrict__ eid,)
    const i64* __restrict__ indices, const T* __restrict__ er, GA_IF_EDGE(const T* __restrict__ ee,)
    const T* __restrict__ V, const T* __restrict__ P, const T* __restrict__ dO, T* __restrict__ del,
    GA_IF_EDGE(T* __restrict__ dee,) i64 n_chunks, i64 h, i64 d, T slope, DropArgsIf<DROP, T> dr) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = row[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  if (j1 <= j0) return;
  for (i64 k = 0; k < h; ++k) {
    T acc = 0;
    for (i64 j = j0 + lane; j < j1; j += kWave) {
      const i64 src = indices[j] GA_IF_EDGE(, e = eid[j]);
      T mult = 1;
      if constexpr (DROP) mult = drop_mult<T>(r, src, k, dr);
      const T dz = GA_FN(dz)<T>(P + (r * h + k) * 4, er[src * h + k], GA_IF_EDGE(ee[e * h + k],) dO + (r * h + k) * d,
                                V + (src * h + k) * d, d, slope, mult);
      GA_IF_EDGE(if (dee) dee[e * h + k] = dz;)
      acc += dz;
    }
    acc = wave_sum(acc);
    if (lane == 0) atomicAdd(del + r * h + k, acc);
  }
}

template <typename T, bool DROP>
__global__ __launch_bounds__(kGenericBlock) void GA_KERNEL(bwd_col, generic)(
    const i64* __restrict__ col, const i64* __restrict__ indptr, GA_IF_EDGE(const i64* __restrict__ eid,)
    const i64* __restrict__ indices, const T* __restrict__ er, GA_IF_EDGE(const T* __restrict__ ee,)
    const T* __restrict__ V, const T* __restrict__ P, const T* __restrict__ dO, T* __restrict__ der,
    T* __restrict__ dV, i64 n_chunks, i64 h, i64 d, T slope, DropArgsIf<DROP, T> dr) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 jc = col[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  if (j1 <= j0) return;
  for (i64 k = 0; k < h; ++k) {   // der: lanes over slots
    T acc = 0;
    for (i64 j = j0 + lane; j < j1; j += kWave) {
      const i64 i = indices[j];
      T mult = 1;
      if constexpr (DROP) mult = drop_mult<T>(i, jc, k, dr);
      acc += GA_FN(dz)<T>(P + (i * h + k) * 4, er[jc * h + k], GA_IF_EDGE(ee[eid[j] * h + k],) dO + (i * h + k) * d,
                          V + (jc * h + k) * d, d, slope, mult);
    }
    acc = wave_sum(acc);
    if (lane == 0) atomicAdd(der + jc * h + k, acc);
  }
  for (i64 it = lane; it < h * d; it += kWave) {   // dV: lanes over the row's values
    const i64 k = it / d;
    T acc = 0;
    for (i64 j = j0; j < j1; ++j) {
      const i64 i = indices[j];
      const T* p = P + (i * h + k) * 4;
      T a = exp_t(gat_lrelu((p[0] + er[jc * h + k]) GA_IF_EDGE(+ ee[eid[j] * h + k]), slope) - p[1]) * p[2];
      if constexpr (DROP) a *= drop_mult<T>(i, jc, k, dr);
      acc += a * dO[i * h * d + it];
    }
    atomicAdd(dV + jc * h * d + it, acc);
  }
}

#undef GA_IF_EDGE
