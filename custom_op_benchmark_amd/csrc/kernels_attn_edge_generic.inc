// The generic passes of the fused dot-product attention ops that add a per-edge row to the key and the value: fp32 /
// fp64, any h and d, any chunk layout; one wave per chunk.  Included twice, inside namespace graphop, after
// kernels_attn_rows_passes.inc and under the AR_EDGE, AR_KERNEL(pass) and AR_FN(name) of that inclusion:
//   kernels_attn_edge.h   AR_EDGE 1  the row of slot j is xe[eid[j]]                         k_attn_edge_*_generic
//   kernels_attn_etype.h  AR_EDGE 2  the row of slot j is R[min(etype[eid[j]], tmax)]        k_attn_etype_*_generic
// The text varies in three things: the parameters that bring the rows (AG_PARAMS), the index of a slot's row in them
// (AG_ROW_OF; the rows themselves are AG_ROWS), and how the row pass delivers the rows' gradient: a slot is visited
// once, so dxe[e] is one plain store, while dR[t] sums over the edges of a type (under `#if AR_EDGE`).
#if AR_EDGE == 1
#define AG_PARAMS(T) const T* __restrict__ xe
#define AG_ROWS xe
#define AG_ROW_OF(j) eid[j]
#else
#define AG_PARAMS(T) const T* __restrict__ R, const int* __restrict__ etype, unsigned tmax
#define AG_ROWS R
#define AG_ROW_OF(j) attn_etype_of(etype, eid[j], tmax)
#endif

// s of one (slot, head): q = Q[i, k, :], kj = K[j, k, :], e = the slot's edge row [k, :].  Every generic pass evaluates
// it by this function, so a recomputed score is bitwise the one the statistics were taken from.
template <typename T>
__device__ __forceinline__ T AR_FN(score)(const T* __restrict__ q, const T* __restrict__ kj, const T* __restrict__ e,
                                          i64 d) {
  T s = 0;
  for (i64 c = 0; c < d; ++c) s += q[c] * (kj[c] + e[c]);
  return s;
}

// stats[i, k] = (-1e9, 0): the floor of the maxima, the start of the sums, and what rows without slots keep
template <typename T>
__global__ void AR_KERNEL(stats_init_generic)(T* __restrict__ stats, i64 n) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { stats[i * 2] = (T)-1e9; stats[i * 2 + 1] = (T)0; }
}
// the sums become 1 / l
template <typename T>
__global__ void AR_KERNEL(stats_fin_generic)(T* __restrict__ stats, i64 n) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { const T s = stats[i * 2 + 1]; stats[i * 2 + 1] = s > (T)0 ? (T)1 / s : (T)0; }
}

// lanes over the chunk's slots, one head at a time; SUM = false: the maxima, true: the sums of exp(s - m)
template <typename T, bool SUM>
__global__ __launch_bounds__(kGenericBlock) void AR_KERNEL(stats_generic)(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ Q, const T* __restrict__ K, AG_PARAMS(T),
    T* __restrict__ stats, i64 n_chunks, i64 h, i64 d) {
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
      const i64 e = AG_ROW_OF(j);
      const T s = AR_FN(score)<T>(Q + (r * h + k) * d, K + (indices[j] * h + k) * d, AG_ROWS + (e * h + k) * d, d);
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
// the two backward kernels): one drop_mult per use, for global head head0 + k.
template <typename T, bool DROP>
__global__ __launch_bounds__(kGenericBlock) void AR_KERNEL(fwd_generic)(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ V,
    AG_PARAMS(T), const T* __restrict__ stats, T* __restrict__ o, i64 n_chunks, i64 h, i64 d, i64 head0,
    DropArgsIf<DROP, T> dr) {
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
      const i64 src = indices[j], e = AG_ROW_OF(j);
      const T s = AR_FN(score)<T>(Q + (r * h + k) * d, K + (src * h + k) * d, AG_ROWS + (e * h + k) * d, d);
      T w = exp_t(s - m) * il;
      if constexpr (DROP) w *= drop_mult<T>(r, src, head0 + k, dr);
      acc += w * (V[src * f + it] + AG_ROWS[e * f + it]);
    }
    atomicAdd(o + r * f + it, acc);
  }
}

// P[i, k] = (m, 1 / l, D = <dO_ik, o_ik>, 0)
template <typename T>
__global__ void AR_KERNEL(pack_generic)(const T* __restrict__ stats, const T* __restrict__ dO, const T* __restrict__ o,
                                        T* __restrict__ P, i64 n, i64 d) {   // n = n_q * h
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  T dsum = 0;
  for (i64 c = 0; c < d; ++c) dsum += dO[i * d + c] * o[i * d + c];
  P[i * 4] = stats[i * 2]; P[i * 4 + 1] = stats[i * 2 + 1]; P[i * 4 + 2] = dsum; P[i * 4 + 3] = 0;
}

// ds of one (slot, head): p = P[i, k] holds (m, 1 / l, D); *a_out = a_e; mult = the slot's dropout multiplier
template <typename T>
__device__ __forceinline__ T AR_FN(ds)(const T* __restrict__ q, const T* __restrict__ kj, const T* __restrict__ vj,
                                       const T* __restrict__ e, const T* __restrict__ p, const T* __restrict__ dO_ik,
                                       i64 d, T mult, T* a_out) {
  const T s = AR_FN(score)<T>(q, kj, e, d);
  const T a = exp_t(s - p[0]) * p[1];
  T da = 0;
  for (i64 t = 0; t < d; ++t) da += dO_ik[t] * (vj[t] + e[t]);
  *a_out = a;
  return a * (mult * da - p[2]);
}

// dx (may be NULL) is the rows' gradient.  AR_EDGE 1: dxe, one store per (slot, element).  AR_EDGE 2: dR, added into
// with global atomics, one per (run of slots of one type, element): a lane sums what consecutive slots of one type give
// before it adds.  The slow path; dR is zero-filled by the caller.
template <typename T, bool DROP>
__global__ __launch_bounds__(kGenericBlock) void AR_KERNEL(bwd_row_generic)(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ V,
    AG_PARAMS(T), const T* __restrict__ P, const T* __restrict__ dO, T* __restrict__ dQ, T* __restrict__ dx,
    i64 n_chunks, i64 h, i64 d, i64 head0, DropArgsIf<DROP, T> dr) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = row[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  if (j1 <= j0) return;
  const i64 f = h * d;
  for (i64 it = lane; it < f; it += kWave) {
    const i64 k = it / d;
    const T q = Q[r * f + it], g = dO[r * f + it];
    T acc = 0, aij;
#if AR_EDGE == 2
    T run = 0;
    i64 t_run = AG_ROW_OF(j0);
#endif
    for (i64 j = j0; j < j1; ++j) {
      const i64 src = indices[j], e = AG_ROW_OF(j);
      T mult = 1;
      if constexpr (DROP) mult = drop_mult<T>(r, src, head0 + k, dr);
      const T ds = AR_FN(ds)<T>(Q + (r * h + k) * d, K + (src * h + k) * d, V + (src * h + k) * d,
                                AG_ROWS + (e * h + k) * d, P + (r * h + k) * 4, dO + (r * h + k) * d, d, mult, &aij);
      acc += ds * (K[src * f + it] + AG_ROWS[e * f + it]);
#if AR_EDGE == 1
      if (dx != nullptr) dx[e * f + it] = ds * q + aij * mult * g;   // a slot is visited once
#else
      if (dx != nullptr) {
        if (e != t_run) { atomicAdd(dx + t_run * f + it, run); run = 0; t_run = e; }
        run += ds * q + aij * mult * g;
      }
#endif
    }
    atomicAdd(dQ + r * f + it, acc);
#if AR_EDGE == 2
    if (dx != nullptr) atomicAdd(dx + t_run * f + it, run);
#endif
  }
}

template <typename T, bool DROP>
__global__ __launch_bounds__(kGenericBlock) void AR_KERNEL(bwd_col_generic)(
    const i64* __restrict__ col, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ V,
    AG_PARAMS(T), const T* __restrict__ P, const T* __restrict__ dO, T* __restrict__ dK, T* __restrict__ dV,
    i64 n_chunks, i64 h, i64 d, i64 head0, DropArgsIf<DROP, T> dr) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 jc = col[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  if (j1 <= j0) return;
  const i64 f = h * d;
  for (i64 it = lane; it < f; it += kWave) {
    const i64 k = it / d;
    T acc_k = 0, acc_v = 0, aij;
    for (i64 j = j0; j < j1; ++j) {
      const i64 i = indices[j], e = AG_ROW_OF(j);
      T mult = 1;
      if constexpr (DROP) mult = drop_mult<T>(i, jc, head0 + k, dr);
      const T ds = AR_FN(ds)<T>(Q + (i * h + k) * d, K + (jc * h + k) * d, V + (jc * h + k) * d,
                                AG_ROWS + (e * h + k) * d, P + (i * h + k) * 4, dO + (i * h + k) * d, d, mult, &aij);
      acc_k += ds * Q[i * f + it];
      acc_v += aij * mult * dO[i * f + it];
    }
    atomicAdd(dK + jc * f + it, acc_k);
    atomicAdd(dV + jc * f + it, acc_v);
  }
}

#undef AG_PARAMS
#undef AG_ROWS
#undef AG_ROW_OF
