// Host side of attention dropout (kernels_dropout.h has the decision): the checked arguments of the *_dropout_* entry
// points as the kernels take them.  Shared by gat_attention.hip and gatv2_attention.hip.  Not part of the C ABI.
#pragma once
#include <cmath>

#include "common.h"
#include "kernels_dropout.h"

namespace graphop {

// the dropout arguments as the host prepares them: T = floor(p * 2^32) and 1 / (1 - p), both computed in double
struct HostDrop {
  unsigned key0, key1, offset, thresh;
  double scale;
  template <typename T>
  DropArgs<T> as() const { return DropArgs<T>{key0, key1, offset, thresh, (T)scale}; }
};

// the kernel argument of a DROP instantiation; drop is NULL exactly where DROP is false
template <bool DROP, typename T>
inline DropArgsIf<DROP, T> drop_arg(const HostDrop* drop) {
  if constexpr (DROP) return drop->as<T>();
  else return NoDrop{};
}

inline int drop_check(const char* fn, double p, uint64_t seed, i64 n_l, i64 n_r, uint32_t offset, HostDrop* out) {
  GO_CHECK_ARG(p >= 0.0 && p < 1.0, "%s: dropout probability p must be in [0, 1), got %g", fn, p);
  GO_CHECK_ARG((seed >> 63) == 0, "%s: seed must be below 2^63, got %llu", fn, (unsigned long long)seed);
  GO_CHECK_ARG(n_l < ((i64)1 << 32) && n_r < ((i64)1 << 32),
               "%s: node ids must fit 32 bits for the dropout counter (n_l=%lld n_r=%lld)", fn, (long long)n_l,
               (long long)n_r);
  out->key0 = (unsigned)(seed & 0xffffffffu);
  out->key1 = (unsigned)(seed >> 32);
  out->offset = offset;
  out->thresh = (unsigned)(uint64_t)std::floor(p * 4294967296.0);
  out->scale = 1.0 / (1.0 - p);
  return GRAPHOP_OK;
}

}  // namespace graphop
