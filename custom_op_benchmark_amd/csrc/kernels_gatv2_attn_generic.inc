// The generic gather passes of the fused GATv2 layer: fp32 / fp64, any h and d, any chunk layout; one wave per chunk.
// kernels_gatv2_attn.h includes this file with GV2_EDGE 0, GV2_GKERNEL(pass) = k_gv2attn_<pass>_generic and
// GV2_GFN(name) = gv2attn_<name>; kernels_gatv2_edge_attn.h with GV2_EDGE 1, k_gv2edge_<pass>_generic and gv2edge_<name>:
// z = (xl_i + xr_j) + xe_e for edge e = eid[slot], and the row pass stores dxe[e] = ds att t where dxe is not NULL.
// GV2_IF_EDGE(...) is its arguments with the edge row and nothing without.
#if GV2_EDGE
#define GV2_IF_EDGE(...) __VA_ARGS__
#else
#define GV2_IF_EDGE(...)
#endif

// s of one (slot, head): a = xl[i, k, :], b = xr[j, k, :], (e = xe[eid, k, :],) w = att[k, :].  Every generic pass
// evaluates it by this function, so a recomputed score is bitwise the one the statistics were taken from.
template <typename T>
__device__ __forceinline__ T GV2_GFN(score)(const T* __restrict__ a, const T* __restrict__ b,
                                            GV2_IF_EDGE(const T* __restrict__ e,) const T* __restrict__ w, i64 d,
                                            T slope) {
  T s = 0;
  for (i64 c = 0; c < d; ++c) s += w[c] * gat_lrelu((a[c] + b[c]) GV2_IF_EDGE(+ e[c]), slope);
  return s;
}

// lanes over the chunk's slots, one head at a time
template <typename T, bool SUM>
__global__ __launch_bounds__(kGenericBlock) void GV2_GKERNEL(stats)(
    const i64* __restrict__ row, const i64* __restrict__ indptr, GV2_IF_EDGE(const i64* __restrict__ eid,)
    const i64* __restrict__ indices, const T* __restrict__ xl, const T* __restrict__ xr,
    GV2_IF_EDGE(const T* __restrict__ xe,) const T* __restrict__ att, T* __restrict__ stats, i64 n_chunks, i64 h, i64 d,
    T slope) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = row[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  if (j1 <= j0) return;   // wave-uniform
  for (i64 k = 0; k < h; ++k) {
    const T m = SUM ? stats[(r * h + k) * 2] : (T)0;
    T acc = SUM ? (T)0 : (T)-1e9;
    for (i64 j = j0 + lane; j < j1; j += kWave) {
      const T s = GV2_GFN(score)<T>(xl + (r * h + k) * d, xr + (indices[j] * h + k) * d,
                                    GV2_IF_EDGE(xe + (eid[j] * h + k) * d,) att + k * d, d, slope);
      if constexpr (SUM) acc += exp_t(s - m);
      else acc = s > acc ? s : acc;
    }
    for (int o = 1; o < kWave; o <<= 1) {
      const T t = __shfl_xor(acc, o);
      if constexpr (SUM) acc += t;
      else acc = t > acc ? t : acc;
    }
    if (lane == 0) {
      if constexpr (SUM) atomicAdd(stats + (r * h + k) * 2 + 1, acc);
      else atomic_max_float(stats + (r * h + k) * 2, acc);
    }
  }
}

// lanes over the h * d elements of the row in steps of the wave; one atomic per (chunk, element).  DROP (here and in
// the two backward kernels): one drop_mult per use.
template <typename T, bool DROP>
__global__ __launch_bounds__(kGenericBlock) void GV2_GKERNEL(fwd)(
    const i64* __restrict__ row, const i64* __restrict__ indptr, GV2_IF_EDGE(const i64* __restrict__ eid,)
    const i64* __restrict__ indices, const T* __restrict__ xl, const T* __restrict__ xr,
    GV2_IF_EDGE(const T* __restrict__ xe,) const T* __restrict__ att, const T* __restrict__ stats, T* __restrict__ o,
    i64 n_chunks, i64 h, i64 d, T slope, DropArgsIf<DROP, T> dr) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = row[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  if (j1 <= j0) return;
  const i64 f = h * d;
  for (i64 it = lane; it < f; it += kWave) {
    const i64 k = it / d;
    const T m = stats[(r * h + k) * 2], il = stats[(r * h + k) * 2 + 1];
    T acc = 0;
    for (i64 j = j0; j < j1; ++j) {
      const i64 src = indices[j];
      const T s = GV2_GFN(score)<T>(xl + (r * h + k) * d, xr + (src * h + k) * d,
                                    GV2_IF_EDGE(xe + (eid[j] * h + k) * d,) att + k * d, d, slope);
      T w = exp_t(s - m) * il;
      if constexpr (DROP) w *= drop_mult<T>(r, src, k, dr);
      acc += w * xr[src * f + it];
    }
    atomicAdd(o + r * f + it, acc);
  }
}

// ds of one (slot, head): i = the row-major row (P[i, k] holds m, 1 / l, D), j = the column; *a_out = a_ij; mult = the
// slot's dropout multiplier m_ij (1 without dropout)
template <typename T>
__device__ __forceinline__ T GV2_GFN(ds)(const T* __restrict__ xl_ik, const T* __restrict__ xr_jk,
                                         GV2_IF_EDGE(const T* __restrict__ xe_ek,) const T* __restrict__ att_k,
                                         const T* __restrict__ p, const T* __restrict__ dO_ik, i64 d, T slope, T mult,
                                         T* a_out) {
  const T s = GV2_GFN(score)<T>(xl_ik, xr_jk, GV2_IF_EDGE(xe_ek,) att_k, d, slope);
  const T a = exp_t(s - p[0]) * p[1];
  T da = 0;
  for (i64 t = 0; t < d; ++t) da += dO_ik[t] * xr_jk[t];
  *a_out = a;
  return a * (mult * da - p[2]);
}

template <typename T, bool DROP>
__global__ __launch_bounds__(kGenericBlock) void GV2_GKERNEL(bwd_row)(
    const i64* __restrict__ row, const i64* __restrict__ indptr, GV2_IF_EDGE(const i64* __restrict__ eid,)
    const i64* __restrict__ indices, const T* __restrict__ xl, const T* __restrict__ xr,
    GV2_IF_EDGE(const T* __restrict__ xe,) const T* __restrict__ att, const T* __restrict__ P,
    const T* __restrict__ dO, T* __restrict__ dxl, GV2_IF_EDGE(T* __restrict__ dxe,) T* __restrict__ datt,
    i64 n_chunks, i64 h, i64 d, T slope, DropArgsIf<DROP, T> dr) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = row[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  if (j1 <= j0) return;
  const i64 f = h * d;
  for (i64 it = lane; it < f; it += kWave) {
    const i64 k = it / d;
    const T a = xl[r * f + it];
    T acc = 0, dw = 0, aij;
    for (i64 j = j0; j < j1; ++j) {
      const i64 src = indices[j] GV2_IF_EDGE(, e = eid[j]);
      T mult = 1;
      if constexpr (DROP) mult = drop_mult<T>(r, src, k, dr);
      const T ds = GV2_GFN(ds)<T>(xl + (r * h + k) * d, xr + (src * h + k) * d, GV2_IF_EDGE(xe + (e * h + k) * d,)
                                  att + k * d, P + (r * h + k) * 4, dO + (r * h + k) * d, d, slope, mult, &aij);
      const T z = (a + xr[src * f + it]) GV2_IF_EDGE(+ xe[e * f + it]);
      acc += gat_lrelu_grad(z, ds, slope);
      dw += ds * gat_lrelu(z, slope);
      GV2_IF_EDGE(if (dxe != nullptr) dxe[e * f + it] = gat_lrelu_grad(z, ds, slope) * att[it];)   // a slot is visited once
    }
    atomicAdd(dxl + r * f + it, acc * att[it]);
    atomicAdd(datt + it, dw);
  }
}

template <typename T, bool DROP>
__global__ __launch_bounds__(kGenericBlock) void GV2_GKERNEL(bwd_col)(
    const i64* __restrict__ col, const i64* __restrict__ indptr, GV2_IF_EDGE(const i64* __restrict__ eid,)
    const i64* __restrict__ indices, const T* __restrict__ xl, const T* __restrict__ xr,
    GV2_IF_EDGE(const T* __restrict__ xe,) const T* __restrict__ att, const T* __restrict__ P,
    const T* __restrict__ dO, T* __restrict__ dxr, i64 n_chunks, i64 h, i64 d, T slope, DropArgsIf<DROP, T> dr) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 jc = col[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  if (j1 <= j0) return;
  const i64 f = h * d;
  for (i64 it = lane; it < f; it += kWave) {
    const i64 k = it / d;
    const T b = xr[jc * f + it], w = att[it];
    T acc = 0, aij;
    for (i64 j = j0; j < j1; ++j) {
      const i64 i = indices[j] GV2_IF_EDGE(, e = eid[j]);
      T mult = 1;
      if constexpr (DROP) mult = drop_mult<T>(i, jc, k, dr);
      const T ds = GV2_GFN(ds)<T>(xl + (i * h + k) * d, xr + (jc * h + k) * d, GV2_IF_EDGE(xe + (e * h + k) * d,)
                                  att + k * d, P + (i * h + k) * 4, dO + (i * h + k) * d, d, slope, mult, &aij);
      if constexpr (DROP) aij *= mult;   // a_ij m_ij
      acc += gat_lrelu_grad((xl[i * f + it] + b) GV2_IF_EDGE(+ xe[e * f + it]), ds, slope) * w + aij * dO[i * f + it];
    }
    atomicAdd(dxr + jc * f + it, acc);
  }
}

#undef GV2_IF_EDGE
