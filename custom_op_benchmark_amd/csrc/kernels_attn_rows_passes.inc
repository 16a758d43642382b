// The several-head chunk-driver passes of the fused dot-product attention ops, with a per-edge score bias or with an edge
// row added to K and V.  Included three times, inside namespace graphop (after kernels_attn_rows.h):
//   kernels_attn_heads.h  AR_EDGE 0  s = <Q_i, K_j> (+ b[e, k], `bool BIAS`)       k_attn_heads_*, AttnHeads*, attn_heads_*
//   kernels_attn_edge.h   AR_EDGE 1  s = <Q_i, K_j + xe[e]>, V_j + xe[e] for V_j   k_attn_edge_*,  AttnEdge*,  attn_edge_*
//   kernels_attn_etype.h  AR_EDGE 2  the same with xe[e] := R[etype[e]]            k_attn_etype_*, AttnEtype*, attn_etype_*
// The includer defines AR_EDGE, AR_KERNEL(pass), AR_TYPE(Name) and AR_FN(name), and undefines them afterwards.
// AR_IF_BIAS(...) is its arguments in the first inclusion and nothing in the others, AR_IF_EDGE(...) the converse;
// AR_IF_XE(...) stands in the second alone, AR_IF_TABLE(...) in the third alone, AR_IF_NO_TABLE(...) in the first two; the
// spots of several lines stand under `#if AR_EDGE`.  What differs: the trailing `bool BIAS` of the template lists (the
// edge kernels keep <H, D, DROP> and <H, D, COL, OWNED, DROP>), b / db against xe / dxe in the parameters, the load of a
// slot's edge id (under BIAS, or always), the slots' h bias values against their edge row offsets, where the term enters
// the score and the values, what dQ accumulates, and the db / dxe store.  Expanding to nothing (rather than a `bool
// EDGE` on a shared __forceinline__ body, which reschedules nearly every kernel: DESIGN.md 4.5h) leaves every kernel of
// both ops instruction for instruction what its own text compiled to.
//
// Layout (AttnRowsCfg<H, D>): a lane group of L = 16 lanes holds the row's F4 float4 pieces, piece p = v * L + l, so a
// per-head dot product is a group_sum<DQ> that leaves the head's score in every lane of the head.  Each lane carries the
// softmax of ITS pieces' heads itself -- (m, l) in the forward, (m, 1 / l, D) and a, ds in the backward are per (lane,
// piece) values -- and no value crosses heads.  Forward and backward reduce a head's dot product by the same dot4 +
// group_sum<DQ> over the same operands, so the backward recomputes the forward's s bit for bit.  With the edge term
// xe[e * F4 + p] is one float4 per (lane, slot, piece), read once with a non-temporal load and added into the K and V
// pieces where they are consumed: kx = K_j + xe[e], vx = V_j + xe[e], each formed once per piece, in this order.
// A NULL eid means eid[slot] == slot (a plan with eid_identity): a kernel-uniform branch.
// With the type table (DESIGN.md 4.5o) the slot's edge row is R[t * F4 + p], t = min(etype[e], tmax) as unsigned values:
// the lane that holds the slot's ids loads the type behind the edge id and from there on carries it where the second
// inclusion carries the edge id, and the piece is an ordinary cached load (the table is 4 T F bytes).  The row pass sums
// dR in a workgroup-wide LDS table tab[t][component][piece] -- a lane group's 16 lanes add into 16 adjacent words -- and
// at its end adds the table's nonzero words into the replica of dR that blockIdx.x % nrep names.  Its groups past the
// last chunk walk no chunk instead of leaving, so that every thread meets the barriers.
#if AR_EDGE
#define AR_IF_EDGE(...) __VA_ARGS__
#define AR_IF_BIAS(...)
#else
#define AR_IF_EDGE(...)
#define AR_IF_BIAS(...) __VA_ARGS__
#endif
#if AR_EDGE == 1
#define AR_IF_XE(...) __VA_ARGS__
#else
#define AR_IF_XE(...)
#endif
#if AR_EDGE == 2
#define AR_IF_TABLE(...) __VA_ARGS__
#define AR_IF_NO_TABLE(...)
#else
#define AR_IF_TABLE(...)
#define AR_IF_NO_TABLE(...) __VA_ARGS__
#endif

// the dropout decision of the call's heads: global head of local head k is head0 + k
struct AR_TYPE(Drop) {
  DropArgs<float> d;
  int head0;
};
template <bool DROP>
using AR_TYPE(DropIf) = std::conditional_t<DROP, AR_TYPE(Drop), NoDrop>;

// Keep bits of a batch's slots.  Lane l works for slot l % SB: it runs Philox for the blocks l / SB, l / SB + L / SB, ...
// of the blocks the global heads head0 .. head0 + H - 1 fall into (one to three), moves the four decisions of a block to
// the local heads' bit positions, and the lanes of a slot OR their bits together.  Returns, in every lane with
// l % SB == u, slot u's bits (bit k = local head k is kept).  (i, j) = (row-major row, neighbour) as in edge_dropout_mask.
template <int H, int SB>
__device__ __forceinline__ int AR_FN(keep_bits)(int l, unsigned i, unsigned j, const AR_TYPE(Drop)& dr) {
  constexpr int L = 16;
  const int b0 = dr.head0 >> 2;
  const int nblk = ((dr.head0 + H + 3) >> 2) - b0;
  int bits = 0;
  for (int t = l / SB; t < nblk; t += L / SB) {
    const int k4 = drop_keep4<float>(i, j, (unsigned)(b0 + t), dr.d);
    const int sh = (b0 + t) * 4 - dr.head0;   // local head of the block's first decision
    bits |= sh >= 0 ? (k4 << sh) : (k4 >> -sh);
  }
#pragma unroll
  for (int s = SB; s < L; s <<= 1) bits |= __shfl_xor(bits, s, L);
  return bits & ((1 << H) - 1);
}

// ---- forward ------------------------------------------------------------------------------------------------------
struct AR_TYPE(FwdArgs) {
  const float* Q;       // [n_q][H][D]   own rows
  const float* K;       // [n_k][H][D]   gathered
  const float* V;       // [n_k][H][D]   gathered
  AR_IF_BIAS(const float* b;)    // [n_edges][H]     by edge id (BIAS)
  AR_IF_XE(const float* xe;)     // [n_edges][H][D]  by edge id, streamed
  AR_IF_TABLE(const float* R; const int* etype; unsigned tmax;)   // [tmax + 1][H][D]; [n_edges] by edge id
  float* o;             // [n_q][H][D]   zero-filled by the caller (pieces are added)
  float* stats;         // [n_q][H][2]   (m, 1 / l); rows without slots keep the caller's fill: (0, 0) of the ops with a
                        //               bias, (-1e9, 0) of the op with an edge term
  int* p_row;           // [2 * groups]  row | first-piece flag, -1 = none (pre-filled)
  float* p_ml;          // [2 * groups][H][2]
  float* p_o;           // [2 * groups][H][D]
};

// The walk of k_attn_bias_fwd_rows_f32 (a lane group takes chunks_per_group consecutive chunks of a rows_sorted plan;
// rows inside the run are normalised and stored, rows shared with a neighbouring group leave as piece records in slot
// 2 * group + {0: continues from the group before, 1: continues into the group after}).  The online softmax is taken
// batch by batch: the heads' maxima over the batch first, one rescale of (l, o) per batch, then one exp per slot.
template <int H, int D, bool DROP AR_IF_BIAS(, bool BIAS)>
__global__ __launch_bounds__(kFastBlock) void AR_KERNEL(fwd_rows_f32)(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, AR_TYPE(FwdArgs) a, i64 n_chunks, int chunks_per_group, AR_TYPE(DropIf)<DROP> dr) {
  using C = AttnRowsCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB;
  constexpr i64 F4 = C::F4;
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  if (c0 >= c1) return;
  const i64 row_before = c0 > 0 ? row[c0 - 1] : -1;
  const i64 row_after = c1 < n_chunks ? row[c1] : -1;
  int kv[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) kv[v] = gat_attn_head<H, D>(v, l);
  float4 q[NV], o_c[NV];
  float m_c[NV], l_c[NV];   // of the piece's head
  auto finish = [&](i64 r) {
    if (r == row_before || r == row_after) {
      const i64 pi = gid * 2 + (r == row_before ? 0 : 1);
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        reinterpret_cast<float4*>(a.p_o)[pi * F4 + v * L + l] = o_c[v];
        if (l % DQ == 0) reinterpret_cast<float2*>(a.p_ml)[pi * H + kv[v]] = make_float2(m_c[v], l_c[v]);
      }
      if (l == 0) a.p_row[pi] = (int)r | (r != row_before ? kWalkFirstPiece : 0);
    } else {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        if (l_c[v] > 0.f) {   // (the same for every head: a row has slots or has none)
          const float mf = fmaxf(m_c[v], -1e9f);
          const float e = attn_rows_exp(m_c[v] - mf);
          const float lsum = l_c[v] * e;
          const float linv = lsum > 0.f ? 1.f / lsum : 0.f;
          const float f = e * linv;
          float4 o = o_c[v];
          o.x *= f; o.y *= f; o.z *= f; o.w *= f;
          reinterpret_cast<float4*>(a.o)[r * F4 + v * L + l] = o;
          if (l % DQ == 0 && lsum > 0.f) reinterpret_cast<float2*>(a.stats)[r * H + kv[v]] = make_float2(mf, linv);
        }
      }
    }
  };
  i64 cur_row = -1;
  for (i64 c = c0; c < c1; ++c) {
    const i64 r = row[c];
    if (r != cur_row) {
      if (cur_row >= 0) finish(cur_row);
      cur_row = r;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        q[v] = ld4(a.Q, r * F4 + v * L + l);
        o_c[v] = make_float4(0.f, 0.f, 0.f, 0.f);
        m_c[v] = kAttnNegBig;
        l_c[v] = 0.f;
      }
    }
    const i64 j0 = indptr[c], j1 = indptr[c + 1];
    for (i64 jb = j0; jb < j1; jb += SB) {
      const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
      // lane l holds the ids of slot l % SB; slots past the end re-read the batch's last slot and are not folded in
      const int t = l % SB;
      const i64 j = jb + (t < nb ? t : nb - 1);
      const int my_src = (int)indices[j];
      int my_e = 0;
      AR_IF_BIAS(if constexpr (BIAS)) my_e = eid ? (int)eid[j] : (int)j;   // kernel-uniform branch
      AR_IF_TABLE(my_e = (int)min((unsigned)a.etype[my_e], a.tmax);)       // from here on the slot's type, clamped
      float4 x0[SB][NV], x1[SB][NV];
      AR_IF_BIAS(float bb[BIAS ? SB : 1][NV];)
      AR_IF_EDGE(i64 eo[SB];)   // the slots' edge rows: e * F4 is 64-bit
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        AR_IF_EDGE(eo[u] = (i64)group_bcast<L, u>(my_e) * F4;)
        const float4* kp = reinterpret_cast<const float4*>(a.K) + src * F4 + l;
        const float4* vp = reinterpret_cast<const float4*>(a.V) + src * F4 + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) { x0[u][v] = kp[v * L]; x1[u][v] = vp[v * L]; }
      });
#if !AR_EDGE
      if constexpr (BIAS) {   // the slots' H bias values, behind the row requests
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          const i64 e = group_bcast<L, u>(my_e);
#pragma unroll
          for (int v = 0; v < NV; ++v) bb[u][v] = a.b[e * H + kv[v]];
        });
      }
#endif
      int keep[DROP ? SB : 1];
      if constexpr (DROP) {
        const int mine = AR_FN(keep_bits)<H, SB>(l, (unsigned)cur_row, (unsigned)my_src, dr);
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          keep[u] = group_bcast<L, u>(mine);
        });
      }
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        float s[SB];
        float mx = m_c[v];
#pragma unroll
        for (int u = 0; u < SB; ++u) {
#if AR_EDGE
          // the edge piece goes into the gathered pieces here: kx in place of K_j, vx in place of V_j
          const float4 xe4 = AR_IF_XE(ld4_nt(a.xe, eo[u] + v * L + l)) AR_IF_TABLE(ld4(a.R, eo[u] + v * L + l));
          x0[u][v] = attn_rows_add4(x0[u][v], xe4);
          x1[u][v] = attn_rows_add4(x1[u][v], xe4);
#endif
          s[u] = group_sum<DQ>(dot4(q[v], x0[u][v]));
          AR_IF_BIAS(if constexpr (BIAS) s[u] += bb[u][v];)
          if (u < nb) mx = fmaxf(mx, s[u]);   // group-uniform
        }
        const float sc = attn_rows_exp(m_c[v] - mx);
        l_c[v] *= sc;
        o_c[v].x *= sc; o_c[v].y *= sc; o_c[v].z *= sc; o_c[v].w *= sc;
        m_c[v] = mx;
#pragma unroll
        for (int u = 0; u < SB; ++u) {
          if (u < nb) {
            const float p = attn_rows_exp(s[u] - mx);
            l_c[v] += p;
            float pm = p;
            if constexpr (DROP) pm = (keep[u] >> kv[v]) & 1 ? p * dr.d.scale : 0.f;
            attn_rows_fma4(o_c[v], pm, x1[u][v]);
          }
        }
      }
    }
  }
  if (cur_row >= 0) finish(cur_row);
}

// ---- merge of the shared rows' pieces: the walk's three kernels with (m, l) per (piece, head) -----------------------
// Mtmp[row, k] starts at kAttnNegBig, Ltmp[row, k] at 0, o is zero where pieces will be added.
__global__ void AR_KERNEL(piece_max)(const int* __restrict__ p_row, const float* __restrict__ p_ml,
                                     float* __restrict__ Mtmp, i64 n, int h) {   // n = pieces * h
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int rec = p_row[i / h];
  if (rec < 0) return;
  atomic_max_float(Mtmp + (i64)(rec & kWalkRowMask) * h + i % h, p_ml[i * 2]);
}
template <int H, int D>
__global__ __launch_bounds__(kFastBlock) void AR_KERNEL(piece_add)(const int* __restrict__ p_row, const float* __restrict__ p_ml,
                                                                   const float* __restrict__ p_o, const float* __restrict__ Mtmp,
                                                                   float* __restrict__ Ltmp, float* __restrict__ o, i64 n) {
  using C = AttnRowsCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ;
  constexpr i64 F4 = C::F4;
  const int l = threadIdx.x % L;
  const i64 i = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  if (i >= n) return;
  const int rec = p_row[i];
  if (rec < 0) return;
  const i64 row = rec & kWalkRowMask;
  float4 v[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int hd = gat_attn_head<H, D>(k, l);
    const float sc = attn_rows_exp(p_ml[(i * H + hd) * 2] - Mtmp[row * H + hd]);
    v[k] = reinterpret_cast<const float4*>(p_o)[i * F4 + k * L + l];
    v[k].x *= sc; v[k].y *= sc; v[k].z *= sc; v[k].w *= sc;
    if (l % DQ == 0) atomicAdd(Ltmp + row * H + hd, p_ml[(i * H + hd) * 2 + 1] * sc);
  }
  atomic_flush_dense<L, NV>(o, row, v, l);
}
template <int H, int D>
__global__ __launch_bounds__(kFastBlock) void AR_KERNEL(piece_fin)(const int* __restrict__ p_row, const float* __restrict__ Mtmp,
                                                                   const float* __restrict__ Ltmp, float* __restrict__ o,
                                                                   float* __restrict__ stats, i64 n) {
  using C = AttnRowsCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ;
  constexpr i64 F4 = C::F4;
  const int l = threadIdx.x % L;
  const i64 i = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  if (i >= n) return;
  const int rec = p_row[i];
  if (rec < 0 || !(rec & kWalkFirstPiece)) return;       // one piece per shared row finishes it
  const i64 row = rec & kWalkRowMask;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int hd = gat_attn_head<H, D>(k, l);
    const float m = Mtmp[row * H + hd];
    const float mf = fmaxf(m, -1e9f);
    const float e = attn_rows_exp(m - mf);
    const float lsum = Ltmp[row * H + hd] * e;
    const float linv = lsum > 0.f ? 1.f / lsum : 0.f;
    const float f = e * linv;
    float4 v = reinterpret_cast<float4*>(o)[row * F4 + k * L + l];
    v.x *= f; v.y *= f; v.z *= f; v.w *= f;
    reinterpret_cast<float4*>(o)[row * F4 + k * L + l] = v;
    if (l % DQ == 0 && lsum > 0.f) reinterpret_cast<float2*>(stats)[row * H + hd] = make_float2(mf, linv);
  }
}

// ---- backward -----------------------------------------------------------------------------------------------------
// (A_r | B_r) -> out[r][2F]; with STATS also st4[r, k] = (m_rk, linv_rk, <B_rk, O_rk>, 0) per head
template <int H, int D, bool STATS>
__global__ __launch_bounds__(kFastBlock) void AR_KERNEL(pack)(
    const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ out, i64 n,
    const float* __restrict__ O, const float* __restrict__ stats2, float4* __restrict__ st4) {
  using C = AttnRowsCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ;
  constexpr i64 F4 = C::F4;
  const int l = threadIdx.x % L;
  const i64 r = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  if (r >= n) return;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const float4 a = ld4(A, r * F4 + v * L + l);
    const float4 b = ld4(B, r * F4 + v * L + l);
    reinterpret_cast<float4*>(out)[r * 2 * F4 + v * L + l] = a;
    reinterpret_cast<float4*>(out)[r * 2 * F4 + F4 + v * L + l] = b;
    if constexpr (STATS) {
      const float dsum = group_sum<DQ>(dot4(b, ld4(O, r * F4 + v * L + l)));
      if (l % DQ == 0) {
        const i64 k = r * H + gat_attn_head<H, D>(v, l);
        st4[k] = make_float4(stats2[k * 2], stats2[k * 2 + 1], dsum, 0.f);
      }
    }
  }
}

//   COL = false: OWN = (Q | dO) packed [n_q][2F], XT = (K | V) packed, out0 = dQ; db / dxe (may be NULL) is written
//   COL = true : OWN = (K | V) packed [n_k][2F], XT = (Q | dO) packed, out0 = dK, out1 = dV; db / dxe is not touched.
//                With the edge term the row xe[eid[slot]] is a random row read of 4 h d bytes per slot here, inherent to
//                an operand indexed by edge id (DESIGN.md 4.5i)
// stats4[i, k] = (m, 1 / l, D, -) per ROW i of the attention matrix and head in both passes.
template <int H, int D, bool COL, bool OWNED, bool DROP AR_IF_BIAS(, bool BIAS)>
__global__ __launch_bounds__(kFastBlock) void AR_KERNEL(bwd_rows_f32)(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const float* __restrict__ OWN, const float* __restrict__ XT,
    const float4* __restrict__ stats4, const float* __restrict__ AR_IF_BIAS(b) AR_IF_XE(xe) AR_IF_TABLE(R),
    AR_IF_TABLE(const int* __restrict__ etype, unsigned tmax, int nrep,) float* __restrict__ out0,
    float* __restrict__ out1, float* __restrict__ AR_IF_BIAS(db) AR_IF_XE(dxe) AR_IF_TABLE(dR), i64 n_chunks,
    int chunks_per_group, AR_TYPE(DropIf)<DROP> dr) {
  using C = AttnRowsCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB;
  constexpr i64 F4 = C::F4;
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  const i64 c0 = AR_IF_NO_TABLE(gid * chunks_per_group) AR_IF_TABLE(min(gid * chunks_per_group, n_chunks));
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  AR_IF_NO_TABLE(if (c0 >= c1) return;)
#if AR_EDGE == 2
  extern __shared__ float tab[];   // [tmax + 1][4][F4], row pass with dR alone (the launch gives it no byte otherwise)
  const int n_tab = COL || dR == nullptr ? 0 : (int)(tmax + 1) * (int)(4 * F4);   // kernel-uniform
  for (int i = threadIdx.x; i < n_tab; i += kFastBlock) tab[i] = 0.f;
  if (n_tab) __syncthreads();
#endif
  i64 row_before = -1, row_after = -1;
  if constexpr (OWNED) {
    if (c0 > 0) row_before = row[c0 - 1];
    if (c1 < n_chunks) row_after = row[c1];
  }
  int kv[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) kv[v] = gat_attn_head<H, D>(v, l);
  float4 y0[NV], y1[NV], acc0[NV], acc1[COL ? NV : 1];
  float4 own_st[COL ? 1 : NV];   // ROW: (m, 1 / l, D) of the piece's head
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
        if constexpr (!COL) own_st[v] = stats4[r * H + kv[v]];
      }
    }
    const i64 j0 = indptr[c], j1 = indptr[c + 1];
    if (j1 > j0) dirty = true;
    for (i64 jb = j0; jb < j1; jb += SB) {
      const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
      // lane l holds the ids of slot l % SB; slots past the end re-read the batch's last slot with weights 0
      const int t = l % SB;
      const i64 j = jb + (t < nb ? t : nb - 1);
      const int my_src = (int)indices[j];
      int my_e = 0;
      AR_IF_BIAS(if constexpr (BIAS)) my_e = eid ? (int)eid[j] : (int)j;   // kernel-uniform branch
      AR_IF_TABLE(my_e = (int)min((unsigned)etype[my_e], tmax);)           // from here on the slot's type, clamped
      float4 x0[SB][NV], x1[SB][NV];
      float4 stg[COL ? SB : 1][NV];   // COL: the gathered row's statistics
      AR_IF_BIAS(float bb[BIAS ? SB : 1][NV]; int ed[BIAS ? SB : 1];)
      AR_IF_EDGE(i64 eo[SB];)
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        AR_IF_EDGE(eo[u] = (i64)group_bcast<L, u>(my_e) * F4;)
        const float4* rowp = reinterpret_cast<const float4*>(XT) + src * (2 * F4) + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) { x0[u][v] = rowp[v * L]; x1[u][v] = rowp[F4 + v * L]; }
        if constexpr (COL) {
#pragma unroll
          for (int v = 0; v < NV; ++v) stg[u][v] = stats4[src * H + kv[v]];
        }
      });
#if !AR_EDGE
      if constexpr (BIAS) {   // the slots' H bias values, behind the row requests
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          ed[u] = group_bcast<L, u>(my_e);
#pragma unroll
          for (int v = 0; v < NV; ++v) bb[u][v] = b[(i64)ed[u] * H + kv[v]];
        });
      }
#endif
      int keep[DROP ? SB : 1];
      if constexpr (DROP) {
        const int mine = COL ? AR_FN(keep_bits)<H, SB>(l, (unsigned)my_src, (unsigned)cur_row, dr)
                             : AR_FN(keep_bits)<H, SB>(l, (unsigned)cur_row, (unsigned)my_src, dr);
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          keep[u] = group_bcast<L, u>(mine);
        });
      }
#pragma unroll
      for (int u = 0; u < SB; ++u) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
#if AR_EDGE
          const float4 xe4 = AR_IF_XE(ld4_nt(xe, eo[u] + v * L + l)) AR_IF_TABLE(ld4(R, eo[u] + v * L + l));
          float4 kx, vx;   // K_j + xe[e], V_j + xe[e]: of the gathered row in the row pass, of the own row in the column pass
          float s, da;
          if constexpr (COL) {
            kx = attn_rows_add4(y0[v], xe4);
            vx = attn_rows_add4(y1[v], xe4);
            s = group_sum<DQ>(dot4(x0[u][v], kx));
            da = group_sum<DQ>(dot4(x1[u][v], vx));
          } else {
            kx = attn_rows_add4(x0[u][v], xe4);
            vx = attn_rows_add4(x1[u][v], xe4);
            s = group_sum<DQ>(dot4(y0[v], kx));
            da = group_sum<DQ>(dot4(y1[v], vx));
          }
#else
          float s = group_sum<DQ>(dot4(y0[v], x0[u][v]));
          float da = group_sum<DQ>(dot4(y1[v], x1[u][v]));
          if constexpr (BIAS) s += bb[u][v];
#endif
          float4 st;
          if constexpr (COL) st = stg[u][v];
          else st = own_st[v];
          float av = u < nb ? expf(s - st.x) * st.y : 0.f;
          float mult = 1.f;
          if constexpr (DROP) mult = (keep[u] >> kv[v]) & 1 ? dr.d.scale : 0.f;
          if constexpr (DROP) da *= mult;
          const float ds = av * (da - st.z);
          if constexpr (DROP) av *= mult;   // from here on av weights dO only: a_e mult_e
          if constexpr (COL) {
            attn_rows_fma4(acc0[v], ds, x0[u][v]);   // dK += ds Q_i
            attn_rows_fma4(acc1[v], av, x1[u][v]);   // dV += a mult dO_i
          } else {
            // kernel-uniform checks: the gradient of b or xe is wanted.  db before the accumulation, dxe after it: the
            // other order moves instructions in the row pass with a bias
#if !AR_EDGE
            if constexpr (BIAS) {   // the head's first lane stores it, real slots only
              if (db != nullptr && u < nb && l % DQ == 0) db[(i64)ed[u] * H + kv[v]] = ds;
            }
#endif
            attn_rows_fma4(acc0[v], ds, AR_IF_BIAS(x0[u][v]) AR_IF_EDGE(kx));   // dQ += ds K_j, or ds kx
#if AR_EDGE
            // dxe: one plain float4 per lane and real slot; dR: four LDS adds, lane groups may meet in a type
            if (AR_IF_XE(dxe) AR_IF_TABLE(dR) != nullptr && u < nb) {
              float4 g = make_float4(ds * y0[v].x, ds * y0[v].y, ds * y0[v].z, ds * y0[v].w);
              attn_rows_fma4(g, av, y1[v]);
              AR_IF_XE(reinterpret_cast<float4*>(dxe)[eo[u] + v * L + l] = g;)
#if AR_EDGE == 2
              float* tp = tab + eo[u] * 4 + v * L + l;
              atomicAdd(tp, g.x); atomicAdd(tp + F4, g.y); atomicAdd(tp + 2 * F4, g.z); atomicAdd(tp + 3 * F4, g.w);
#endif
            }
#endif
          }
        }
      }
    }
  }
  if (dirty) flush(cur_row);
#if AR_EDGE == 2
  if (n_tab) {   // element i = (t, piece, component) of dR from word (t, component, piece) of the table
    __syncthreads();
    float* rep = dR + (i64)(blockIdx.x % nrep) * n_tab;
    for (int i = threadIdx.x; i < n_tab; i += kFastBlock) {
      const int f = i % (int)(4 * F4);
      const float g = tab[i - f + (f % 4) * (int)F4 + f / 4];
      if (g != 0.f) atomicAdd(rep + i, g);   // a type this workgroup met in no slot adds nothing
    }
  }
#endif
}

#undef AR_IF_EDGE
#undef AR_IF_BIAS
#undef AR_IF_XE
#undef AR_IF_TABLE
#undef AR_IF_NO_TABLE
