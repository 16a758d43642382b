// graphop_cpp: the reference's operator boundary as a compiled PyTorch-ROCm C++ extension.
//
// Same shape as the reference's graphop/graphop.cpp (:1-225): CHECK_CUDA / CHECK_CONTIGUOUS on every
// input (:4-6), eight functions on at::Tensor with the reference's positional signatures and return
// types (:16-30, :39-51, :59-69, :79-93, :108-131, :141-154, :163-175, :190-214), exported twice:
//   * PYBIND11_MODULE  -> importable module (the reference's only registration, :216-225)
//   * TORCH_LIBRARY(graphop, ...) -> torch.ops.graphop.* (north_star's surface; the reference has none)
// Where the reference forwards to its *_cuda_* launchers, this file forwards to the C ABI of
// libgraphop_hip.so (include/graphop_hip.h) on the current HIP stream.  It owns a per-graph plan cache
// (graphop_plan_create is the setup path: validation + derived arrays) under the same byte budget as
// the ctypes binding's; everything else --
// kernels, dispatch, workspaces' layout -- lives behind the C ABI.  The ctypes binding
// (custom_op_benchmark_amd/graphop.py) is the same boundary without a compiler.
#include <torch/extension.h>
#include <torch/library.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <list>
#include <memory>
#include <mutex>
#include <tuple>
#include <unordered_map>

#include "graphop_hip.h"

#define CHECK_CUDA(x) TORCH_CHECK((x).is_cuda(), #x " must be a CUDA tensor")            // graphop.cpp:4
#define CHECK_CONTIGUOUS(x) TORCH_CHECK((x).is_contiguous(), #x " must be contiguous")   // graphop.cpp:5
#define CHECK_INPUT(x) CHECK_CUDA(x); CHECK_CONTIGUOUS(x)                                // graphop.cpp:6
#define CHECK_INDEX(x) TORCH_CHECK((x).scalar_type() == at::kLong, "expected scalar type Long but found ", (x).scalar_type(), " (" #x ")")
// the index arrays of one CSR orientation, with and without `indices`; macros, so that the messages carry the caller's
// spelling of each argument ("indptr_t must be contiguous", "... (eid_c)")
#define CHECK_CSR3(row, indptr, eid) \
  CHECK_INPUT(row); CHECK_INPUT(indptr); CHECK_INPUT(eid); CHECK_INDEX(row); CHECK_INDEX(indptr); CHECK_INDEX(eid)
#define CHECK_CSR(row, indptr, eid, indices)                                     \
  CHECK_INPUT(row); CHECK_INPUT(indptr); CHECK_INPUT(eid); CHECK_INPUT(indices); \
  CHECK_INDEX(row); CHECK_INDEX(indptr); CHECK_INDEX(eid); CHECK_INDEX(indices)
// every value operand of one call has one dtype (the reference's data<scalar_t>() throws otherwise): the C ABI takes
// raw pointers plus ONE dtype code, so a mismatch here would be an out-of-bounds access on the device
#define CHECK_SAME_DTYPE(a, b) TORCH_CHECK((a).scalar_type() == (b).scalar_type(), "expected " #a " and " #b " to have the same dtype, got ", (a).scalar_type(), " and ", (b).scalar_type())
#define CHECK_EDGE_ROWS(x, e) TORCH_CHECK((x).dim() >= 1 && (x).size(0) >= (e), #x " must hold one entry per edge id: ", (x).size(0), " rows for ", (e), " edges")

namespace {

void check(int rc) { TORCH_CHECK(rc == GRAPHOP_OK, "graphop: ", graphop_last_error()); }

int dtype_code(const at::Tensor& t) {
  if (t.scalar_type() == at::kFloat) return GRAPHOP_F32;
  if (t.scalar_type() == at::kDouble) return GRAPHOP_F64;
  TORCH_CHECK(false, "graphop: not implemented for '", t.scalar_type(), "' (float32 / float64 only)");   // AT_DISPATCH_FLOATING_TYPES, graphop_kernel.cu:291
}

void* stream_of(const at::Tensor& t) { return (void*)c10::hip::getCurrentHIPStream(t.get_device()).stream(); }

const int64_t* ip(const at::Tensor& t) { return t.numel() ? t.data_ptr<int64_t>() : nullptr; }
void* vp(const at::Tensor& t) { return t.numel() ? t.data_ptr() : nullptr; }

// ---- plans: least-recently-used cache keyed by the identity and version of the index tensors ----------
// Two levels like the ctypes binding (_lib.get_plan): an entry per (row, indptr, eid) holds the plans of
// that orientation by `indices` tensor; a request without indices (softmax, node_mul_edge) reuses any
// of them.  Entries are handed out as shared_ptr: an eviction by another thread never destroys a plan
// an op is still using.  Budget: kMaxGraphs entries AND the library's device-byte count
// (graphop_memory_bytes: plans of BOTH bindings) against GRAPHOP_PLAN_CACHE_GB (default 96).
struct PlanKey {
  const void *row, *indptr, *eid;
  int64_t n_chunks, n_edges;
  uint32_t v0, v1, v2;
  int device;
  bool operator==(const PlanKey& o) const {
    return row == o.row && indptr == o.indptr && eid == o.eid && n_chunks == o.n_chunks && n_edges == o.n_edges &&
           v0 == o.v0 && v1 == o.v1 && v2 == o.v2 && device == o.device;
  }
};
struct PlanKeyHash {
  size_t operator()(const PlanKey& k) const {
    size_t h = std::hash<const void*>()(k.row);
    for (const void* p : {k.indptr, k.eid}) h = h * 1000003u ^ std::hash<const void*>()(p);
    return h ^ (size_t)k.n_edges ^ ((size_t)k.v0 << 7) ^ ((size_t)k.v2 << 13);
  }
};
struct PlanEntry {
  graphop_plan_t* plan = nullptr;
  graphop_plan_info_t info;
  const void* indices = nullptr;
  uint32_t v_indices = 0;
  std::vector<at::Tensor> keep;   // the arrays the plan points into stay alive with it
  ~PlanEntry() { if (plan) graphop_plan_destroy(plan); }
};
using PlanRef = std::shared_ptr<PlanEntry>;
struct GraphEntry {
  std::vector<PlanRef> plans;     // one per indices tensor (usually one)
  std::list<PlanKey>::iterator lru;
};
std::mutex g_mu;
std::unordered_map<PlanKey, GraphEntry, PlanKeyHash> g_graphs;
std::list<PlanKey> g_lru;
constexpr size_t kMaxGraphs = 64;
int64_t cache_budget_bytes() {
  static const int64_t b = [] {
    const char* v = getenv("GRAPHOP_PLAN_CACHE_GB");
    return (int64_t)((v && *v ? atof(v) : 96.0) * (double)(1LL << 30));
  }();
  return b;
}

PlanRef get_plan(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                 const at::Tensor* indices, int64_t bound) {
  PlanKey k{row.numel() ? row.data_ptr() : nullptr, indptr.data_ptr(), eid.numel() ? eid.data_ptr() : nullptr,
            row.numel(), eid.numel(), (uint32_t)row._version(), (uint32_t)indptr._version(), (uint32_t)eid._version(),
            (int)indptr.get_device()};
  const void* ix = indices && indices->numel() ? indices->data_ptr() : nullptr;
  PlanRef found;
  std::vector<PlanRef> evicted;   // destroyed after the lock is released (plan destruction frees device memory)
  {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_graphs.find(k);
    if (it != g_graphs.end()) {
      g_lru.splice(g_lru.begin(), g_lru, it->second.lru);
      for (auto& p : it->second.plans)
        if (!indices || (p->indices == ix && p->v_indices == (uint32_t)indices->_version())) { found = p; break; }
    }
    if (!found) {
      while (!g_lru.empty() && (g_graphs.size() >= kMaxGraphs || graphop_memory_bytes() > cache_budget_bytes())) {
        if (it != g_graphs.end() && g_lru.back() == k) break;      // never the graph being served
        auto victim = g_graphs.find(g_lru.back());
        for (auto& p : victim->second.plans) evicted.push_back(std::move(p));
        g_graphs.erase(victim);
        g_lru.pop_back();
        bool any_left = false;
        for (auto& e : evicted) any_left |= e.use_count() > 1;
        if (any_left) break;   // still in use elsewhere: its memory will not come back by evicting more
      }
    }
  }
  evicted.clear();
  if (!found) {
    auto e = std::make_shared<PlanEntry>();
    check(graphop_plan_create(ip(row), ip(indptr), ip(eid), indices ? ip(*indices) : nullptr, row.numel(), eid.numel(),
                              bound, stream_of(indptr), &e->plan));   // (not under g_mu: the allocator hook may need the GIL)
    check(graphop_plan_info(e->plan, &e->info));
    e->indices = ix;
    e->v_indices = indices ? (uint32_t)indices->_version() : 0;
    e->keep = {row, indptr, eid};
    if (indices) e->keep.push_back(*indices);
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_graphs.find(k);
    if (it == g_graphs.end()) {
      g_lru.push_front(k);
      GraphEntry ge;
      ge.lru = g_lru.begin();
      it = g_graphs.emplace(k, std::move(ge)).first;
    }
    if (indices) {   // a plan with indices supersedes an index-less one of the same orientation
      auto& v = it->second.plans;
      v.erase(std::remove_if(v.begin(), v.end(), [](const PlanRef& p) { return p->indices == nullptr; }), v.end());
    }
    it->second.plans.push_back(e);
    found = e;
  }
  TORCH_CHECK(!indices || bound <= 0 || found->info.max_index < bound, "graphop: indices holds ", found->info.max_index,
              " but the gathered tensor has only ", bound, " rows");
  return found;
}
PlanRef get_plan(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid, const at::Tensor& indices,
                 int64_t bound) {
  return get_plan(row, indptr, eid, &indices, bound);
}
PlanRef get_plan3(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid) {
  return get_plan(row, indptr, eid, nullptr, 0);
}

struct DeviceGuard {   // the reference calls cudaSetDevice without restoring (graphop_kernel.cu:277)
  c10::DeviceGuard g;
  explicit DeviceGuard(const at::Tensor& t) : g(t.device()) {}
};

at::Tensor edge_out(const at::Tensor& like, int64_t e, int64_t h) {   // (e) if h == 1 else (e, h), graphop_kernel.cu:284
  return h == 1 ? at::empty({e}, like.options()) : at::empty({e, h}, like.options());
}

std::vector<int64_t> with_rows(const at::Tensor& V, int64_t n_rows) {   // o of the fused GAT layers: V's layout, n_src rows
  std::vector<int64_t> shape(V.sizes().begin(), V.sizes().end());
  shape[0] = n_rows;
  return shape;
}

// the row-pass partials of the GATv2 backwards, in values: the workspace minimum of include/graphop_hip.h
int64_t gatv2_row_pass_values(int64_t n_row_chunks, int64_t h, int64_t d) {
  return std::min<int64_t>((n_row_chunks + 15) / 16, 8192) * h * d;
}

// what a fused backward saved from its forward, o (oshape) and stats (n_src, h, 2), and the gradient of o -> that
// gradient, contiguous
at::Tensor saved_checked(const char* fn, at::IntArrayRef oshape, int64_t n_src, int64_t h, const at::Tensor& o,
                         const at::Tensor& stats, const at::Tensor& dO_) {
  TORCH_CHECK(o.sizes() == oshape && stats.numel() == n_src * h * 2, fn, ": o must be ", oshape,
              " and stats (n_src, h, 2), got ", o.sizes(), " and ", stats.sizes());
  at::Tensor dO = dO_.contiguous();
  TORCH_CHECK(dO.sizes() == o.sizes(), fn, ": dO must match o ", o.sizes(), ", got ", dO.sizes());
  return dO;
}

}  // namespace

// ---- the eight functions (graphop.cpp:16-214) ------------------------------------------------------
at::Tensor maskedmm_csr_forward(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                                const at::Tensor& indices, const at::Tensor& A, const at::Tensor& B) {
  CHECK_CSR(row, indptr, eid, indices);
  CHECK_INPUT(A); CHECK_INPUT(B);
  CHECK_SAME_DTYPE(A, B);
  DeviceGuard dg(A);
  const int64_t e = eid.size(0), d = A.size(-1), h = A.dim() == 2 ? 1 : A.size(1);   // graphop_kernel.cu:282-283
  auto y = edge_out(A, e, h);
  const auto pp = get_plan(row, indptr, eid, indices, B.size(0));
  const auto& p = *pp;
  check(graphop_maskedmm_csr_forward(dtype_code(A), ip(row), ip(indptr), ip(eid), ip(indices), vp(A), vp(B), vp(y),
                                     row.size(0), e, A.size(0), B.size(0), h, d, p.plan, stream_of(A)));
  return y;
}

std::vector<at::Tensor> maskedmm_csr_backward(const at::Tensor& row, const at::Tensor& indptr_r,
                                              const at::Tensor& eid_r, const at::Tensor& indices_r,
                                              const at::Tensor& col, const at::Tensor& indptr_c,
                                              const at::Tensor& eid_c, const at::Tensor& indices_c,
                                              const at::Tensor& A, const at::Tensor& B, const at::Tensor& dy_) {
  CHECK_CSR(row, indptr_r, eid_r, indices_r);
  CHECK_CSR(col, indptr_c, eid_c, indices_c);
  CHECK_INPUT(A); CHECK_INPUT(B);
  CHECK_CUDA(dy_);
  const at::Tensor dy = dy_.contiguous();   // the reference forgets this check (graphop.cpp:120-129)
  CHECK_SAME_DTYPE(A, B); CHECK_SAME_DTYPE(A, dy); CHECK_EDGE_ROWS(dy, eid_r.size(0));
  DeviceGuard dg(A);
  const int64_t d = A.size(-1), h = dy.dim() == 2 ? dy.size(1) : 1;   // graphop_kernel.cu:373
  auto dA = at::empty_like(A), dB = at::empty_like(B);
  const auto ppr = get_plan(row, indptr_r, eid_r, indices_r, B.size(0));
  const auto ppc = get_plan(col, indptr_c, eid_c, indices_c, A.size(0));
  const auto &pr = *ppr, &pc = *ppc;
  check(graphop_maskedmm_csr_backward(dtype_code(A), ip(row), ip(indptr_r), ip(eid_r), ip(indices_r), ip(col),
                                      ip(indptr_c), ip(eid_c), ip(indices_c), vp(A), vp(B), vp(dy), vp(dA), vp(dB),
                                      row.size(0), col.size(0), eid_r.size(0), A.size(0), B.size(0), h, d, pr.plan,
                                      pc.plan, stream_of(A)));
  return {dA, dB};
}

at::Tensor node_mul_edge_forward(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                                 const at::Tensor& A, const at::Tensor& B) {
  CHECK_CSR3(row, indptr, eid);
  CHECK_INPUT(A); CHECK_INPUT(B);
  CHECK_SAME_DTYPE(A, B);
  DeviceGuard dg(A);
  const int64_t e = eid.size(0), d = A.size(-1), h = A.dim() == 2 ? 1 : A.size(1);
  TORCH_CHECK(B.size(0) >= e && B.size(-1) == d, "node_mul_edge_forward: B must be (n_edges, d)");
  auto y = edge_out(A, e, h);
  const auto pp = get_plan3(row, indptr, eid);
  const auto& p = *pp;
  check(graphop_node_mul_edge_forward(dtype_code(A), ip(row), ip(indptr), ip(eid), vp(A), vp(B), vp(y), row.size(0), e,
                                      A.size(0), h, d, p.plan, stream_of(A)));
  return y;
}

std::vector<at::Tensor> node_mul_edge_backward(const at::Tensor& row, const at::Tensor& indptr,
                                               const at::Tensor& eid, const at::Tensor& A, const at::Tensor& B,
                                               const at::Tensor& dy_) {
  CHECK_CSR3(row, indptr, eid);
  CHECK_INPUT(A); CHECK_INPUT(B);
  CHECK_CUDA(dy_);
  const at::Tensor dy = dy_.contiguous();
  CHECK_SAME_DTYPE(A, B); CHECK_SAME_DTYPE(A, dy); CHECK_EDGE_ROWS(dy, eid.size(0));
  DeviceGuard dg(A);
  const int64_t e = eid.size(0), d = A.size(-1), h = dy.dim() == 2 ? dy.size(1) : 1;
  TORCH_CHECK(B.size(0) == e && B.size(-1) == d, "node_mul_edge_backward: B must be (n_edges, d)");
  auto dA = at::empty_like(A), dB = at::empty_like(B);
  const auto pp = get_plan3(row, indptr, eid);
  const auto& p = *pp;
  check(graphop_node_mul_edge_backward(dtype_code(A), ip(row), ip(indptr), ip(eid), vp(A), vp(B), vp(dy), vp(dA),
                                       vp(dB), row.size(0), e, A.size(0), h, d, p.plan, stream_of(A)));
  return {dA, dB};
}

at::Tensor sparse_softmax_forward(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                                  const at::Tensor& x) {
  CHECK_CSR3(row, indptr, eid);
  CHECK_INPUT(x);
  CHECK_EDGE_ROWS(x, eid.size(0));
  DeviceGuard dg(x);
  const int64_t h = x.dim() == 2 ? x.size(1) : 1;
  auto y = at::empty_like(x);
  const auto pp = get_plan3(row, indptr, eid);
  const auto& p = *pp;
  at::Tensor ws;
  int64_t ws_rows = 0;
  if (!p.info.row_owned) {   // general layout: max / sum scratch per row (the reference sizes it by E, :426-427)
    ws_rows = p.info.max_row + 1;
    ws = at::empty({2 * ws_rows * h}, x.options());
  }
  check(graphop_sparse_softmax_forward(dtype_code(x), ip(row), ip(indptr), ip(eid), vp(x), vp(y), row.size(0),
                                       eid.size(0), h, ws.defined() ? vp(ws) : nullptr, ws_rows, p.plan, stream_of(x)));
  return y;
}

at::Tensor sparse_softmax_backward(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                                   const at::Tensor& y, const at::Tensor& dy_) {
  CHECK_CSR3(row, indptr, eid);
  CHECK_INPUT(y);
  CHECK_CUDA(dy_);
  const at::Tensor dy = dy_.contiguous();
  CHECK_SAME_DTYPE(y, dy); CHECK_EDGE_ROWS(y, eid.size(0)); CHECK_EDGE_ROWS(dy, eid.size(0));
  TORCH_CHECK(y.sizes() == dy.sizes(), "sparse_softmax_backward: y and dy must have the same shape");
  DeviceGuard dg(y);
  const int64_t h = dy.dim() == 2 ? dy.size(1) : 1;
  auto dx = at::empty_like(dy);
  const auto pp = get_plan3(row, indptr, eid);
  const auto& p = *pp;
  at::Tensor ws;
  int64_t ws_rows = 0;
  if (!p.info.row_owned) {
    ws_rows = p.info.max_row + 1;
    ws = at::empty({ws_rows * h}, y.options());
  }
  check(graphop_sparse_softmax_backward(dtype_code(y), ip(row), ip(indptr), ip(eid), vp(y), vp(dy), vp(dx), row.size(0),
                                        eid.size(0), h, ws.defined() ? vp(ws) : nullptr, ws_rows, p.plan, stream_of(y)));
  return dx;
}

at::Tensor vector_spmm_forward(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                               const at::Tensor& indices, const at::Tensor& edata, const at::Tensor& x) {
  CHECK_CSR(row, indptr, eid, indices);
  CHECK_INPUT(edata); CHECK_INPUT(x);
  CHECK_SAME_DTYPE(edata, x); CHECK_EDGE_ROWS(edata, eid.size(0));
  DeviceGuard dg(x);
  const int64_t h = edata.dim() == 2 ? edata.size(1) : 1, d = x.size(-1);   // graphop_kernel.cu:520
  auto y = at::empty_like(x);                                               // zeros_like(x), :527
  const auto pp = get_plan(row, indptr, eid, indices, x.size(0));
  const auto& p = *pp;
  check(graphop_vector_spmm_forward(dtype_code(x), ip(row), ip(indptr), ip(eid), ip(indices), vp(edata), vp(x), vp(y),
                                    row.size(0), eid.size(0), x.size(0), x.size(0), h, d, p.plan, stream_of(x)));
  return y;
}

std::vector<at::Tensor> vector_spmm_backward(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                                             const at::Tensor& indices, const at::Tensor& col,
                                             const at::Tensor& indptr_t, const at::Tensor& eid_t,
                                             const at::Tensor& indices_t, const at::Tensor& edata,
                                             const at::Tensor& dy, const at::Tensor& x) {   // NB dy before x, graphop.cpp:199-201
  CHECK_CSR(row, indptr, eid, indices);
  CHECK_CSR(col, indptr_t, eid_t, indices_t);
  CHECK_INPUT(edata); CHECK_INPUT(dy); CHECK_INPUT(x);
  CHECK_SAME_DTYPE(edata, x); CHECK_SAME_DTYPE(dy, x); CHECK_EDGE_ROWS(edata, eid.size(0));
  DeviceGuard dg(x);
  const int64_t h = edata.dim() == 2 ? edata.size(1) : 1, d = x.size(-1);
  auto dedata = at::empty_like(edata), dx = at::empty_like(x);
  const auto ppr = get_plan(row, indptr, eid, indices, x.size(0));
  const auto ppc = get_plan(col, indptr_t, eid_t, indices_t, dy.size(0));
  const auto &pr = *ppr, &pc = *ppc;
  check(graphop_vector_spmm_backward(dtype_code(x), ip(row), ip(indptr), ip(eid), ip(indices), ip(col), ip(indptr_t),
                                     ip(eid_t), ip(indices_t), vp(edata), vp(dy), vp(x), vp(dedata), vp(dx),
                                     row.size(0), col.size(0), eid.size(0), x.size(0), dy.size(0), h, d, pr.plan,
                                     pc.plan, stream_of(x)));
  return {dedata, dx};   // graphop_kernel.cu:599
}

// (p, seed, offset) of the dropout forms, checked as include/graphop_hip.h states them
struct DropSpec {
  double p;
  uint64_t seed;
  uint32_t offset;
};

DropSpec drop_spec(const char* fn, double p, int64_t seed, int64_t offset) {
  TORCH_CHECK(p >= 0.0 && p < 1.0, fn, ": dropout probability p must be in [0, 1), got ", p);
  TORCH_CHECK(seed >= 0, fn, ": seed must be in [0, 2^63), got ", seed);
  TORCH_CHECK(offset >= 0 && offset < (int64_t(1) << 32), fn, ": offset must be in [0, 2^32), got ", offset);
  return {p, (uint64_t)seed, (uint32_t)offset};
}

// ---- the extra fused op (include/graphop_hip.h: graphop_attention_*) ------------------------------
void check_attn_bias_input(const at::Tensor& b) { CHECK_INPUT(b); }
// b of the forms with a per-edge score bias: (n_edges) for 2-D Q / K / V, else (n_edges, h), in Q's dtype
void check_attn_bias(const char* fn, const at::Tensor& b, const at::Tensor& Q, int64_t e, int64_t h) {
  CHECK_SAME_DTYPE(Q, b); CHECK_EDGE_ROWS(b, e);
  TORCH_CHECK(Q.dim() == 2 ? (b.dim() == 1 && b.size(0) == e) : (b.dim() == 2 && b.size(0) == e && b.size(1) == h),
              fn, ": b must be (n_edges) for 2-D Q / K / V, else (n_edges, h) with n_edges = ", e, " and h = ", h,
              ", got b ", b.sizes(), ", Q ", Q.sizes());
}

// drop == nullptr: graphop_attention_forward, else its dropout form for the heads head0 .. head0 + h - 1, as `fn`;
// b != nullptr (with drop given): the form with a per-edge score bias
std::vector<at::Tensor> attention_forward_impl(const char* fn, const at::Tensor& row, const at::Tensor& indptr,
                                               const at::Tensor& eid, const at::Tensor& indices, const at::Tensor& Q,
                                               const at::Tensor& K, const at::Tensor& V, const DropSpec* drop,
                                               int64_t head0, const at::Tensor* b = nullptr) {
  CHECK_CSR(row, indptr, eid, indices);
  CHECK_INPUT(Q); CHECK_INPUT(K); CHECK_INPUT(V);
  if (b) check_attn_bias_input(*b);
  TORCH_CHECK(K.sizes() == V.sizes() && Q.sizes().slice(1) == K.sizes().slice(1),
              fn, ": Q (n_q,[h,]d), K and V (n_k,[h,]d) expected");
  CHECK_SAME_DTYPE(Q, K); CHECK_SAME_DTYPE(Q, V);
  DeviceGuard dg(Q);
  const int64_t e = eid.size(0), d = Q.size(-1), h = Q.dim() == 2 ? 1 : Q.size(1), n_q = Q.size(0), n_k = K.size(0);
  auto o = at::empty_like(Q);
  auto stats = at::empty({n_q, h, 2}, Q.options());
  const auto pp = get_plan(row, indptr, eid, indices, n_k);
  const auto& p = *pp;
  int64_t nbytes = 0;
  if (b) {
    check_attn_bias(fn, *b, Q, e, h);
    check(graphop_attention_bias_workspace_bytes(dtype_code(Q), 0, e, n_q, n_k, h, d, p.plan, nullptr, stream_of(Q), 0, &nbytes));
  } else {
    check((drop ? graphop_attention_dropout_workspace_bytes : graphop_attention_workspace_bytes)(
        dtype_code(Q), 0, e, n_q, n_k, h, d, p.plan, nullptr, stream_of(Q), &nbytes));
  }
  auto ws = at::empty({std::max<int64_t>(nbytes, 1)}, Q.options().dtype(at::kByte));
  if (b)
    check(graphop_attention_bias_forward(dtype_code(Q), ip(row), ip(indptr), ip(eid), ip(indices), vp(Q), vp(K), vp(V),
                                         vp(*b), vp(o), vp(stats), row.size(0), e, n_q, n_k, h, d, ws.data_ptr(), nbytes,
                                         p.plan, stream_of(Q), drop->p, drop->seed, drop->offset, head0));
  else if (drop)
    check(graphop_attention_dropout_forward(dtype_code(Q), ip(row), ip(indptr), ip(eid), ip(indices), vp(Q), vp(K), vp(V),
                                            vp(o), vp(stats), row.size(0), e, n_q, n_k, h, d, ws.data_ptr(), nbytes,
                                            p.plan, stream_of(Q), drop->p, drop->seed, drop->offset, head0));
  else
    check(graphop_attention_forward(dtype_code(Q), ip(row), ip(indptr), ip(eid), ip(indices), vp(Q), vp(K), vp(V), vp(o),
                                    vp(stats), row.size(0), e, n_q, n_k, h, d, ws.data_ptr(), nbytes, p.plan, stream_of(Q)));
  return {o, stats};
}

std::vector<at::Tensor> attention_forward(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                                          const at::Tensor& indices, const at::Tensor& Q, const at::Tensor& K,
                                          const at::Tensor& V) {
  return attention_forward_impl("attention_forward", row, indptr, eid, indices, Q, K, V, nullptr, 0);
}

// head0 of the dropout forms: the global index of the call's first head
int64_t head0_checked(const char* fn, int64_t head0) {
  TORCH_CHECK(head0 >= 0 && head0 < (int64_t(1) << 32), fn, ": head0 must be in [0, 2^32), got ", head0);
  return head0;
}

std::vector<at::Tensor> attention_dropout_forward(const at::Tensor& row, const at::Tensor& indptr,
                                                  const at::Tensor& eid, const at::Tensor& indices, const at::Tensor& Q,
                                                  const at::Tensor& K, const at::Tensor& V, double p, int64_t seed,
                                                  int64_t offset, int64_t head0) {
  const char* fn = "attention_dropout_forward";
  const DropSpec drop = drop_spec(fn, p, seed, offset);
  return attention_forward_impl(fn, row, indptr, eid, indices, Q, K, V, &drop, head0_checked(fn, head0));
}

std::vector<at::Tensor> attention_bias_forward(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                                               const at::Tensor& indices, const at::Tensor& Q, const at::Tensor& K,
                                               const at::Tensor& V, const at::Tensor& b, double p, int64_t seed,
                                               int64_t offset, int64_t head0) {
  const char* fn = "attention_bias_forward";
  const DropSpec drop = drop_spec(fn, p, seed, offset);
  return attention_forward_impl(fn, row, indptr, eid, indices, Q, K, V, &drop, head0_checked(fn, head0), &b);
}

// drop == nullptr: graphop_attention_backward, else its dropout form, as `fn`; b != nullptr (with drop given): the form
// with a per-edge score bias, which returns db as a fourth tensor (empty with need_db == false)
std::vector<at::Tensor> attention_backward_impl(const char* fn, const at::Tensor& row, const at::Tensor& indptr_r,
                                                const at::Tensor& eid_r, const at::Tensor& indices_r,
                                                const at::Tensor& col, const at::Tensor& indptr_c,
                                                const at::Tensor& eid_c, const at::Tensor& indices_c,
                                                const at::Tensor& Q, const at::Tensor& K, const at::Tensor& V,
                                                const at::Tensor& o, const at::Tensor& stats, const at::Tensor& dO_,
                                                const DropSpec* drop, int64_t head0, const at::Tensor* b = nullptr,
                                                bool need_db = true) {
  CHECK_CSR(row, indptr_r, eid_r, indices_r);
  CHECK_CSR(col, indptr_c, eid_c, indices_c);
  CHECK_INPUT(Q); CHECK_INPUT(K); CHECK_INPUT(V);
  if (b) check_attn_bias_input(*b);
  CHECK_INPUT(o); CHECK_INPUT(stats);
  CHECK_CUDA(dO_);
  const at::Tensor dO = dO_.contiguous();
  CHECK_SAME_DTYPE(Q, K); CHECK_SAME_DTYPE(Q, V); CHECK_SAME_DTYPE(Q, o); CHECK_SAME_DTYPE(Q, stats); CHECK_SAME_DTYPE(Q, dO);
  TORCH_CHECK(K.sizes() == V.sizes() && Q.sizes().slice(1) == K.sizes().slice(1),
              fn, ": Q (n_q,[h,]d), K and V (n_k,[h,]d) expected");
  DeviceGuard dg(Q);
  const int64_t e = eid_r.size(0), d = Q.size(-1), h = Q.dim() == 2 ? 1 : Q.size(1), n_q = Q.size(0), n_k = K.size(0);
  TORCH_CHECK(o.sizes() == Q.sizes() && dO.sizes() == Q.sizes() && stats.numel() == n_q * h * 2,
              fn, ": o, dO must match Q and stats must be (n_q, h, 2)");
  auto dQ = at::empty_like(Q), dK = at::empty_like(K), dV = at::empty_like(V);
  const auto ppr = get_plan(row, indptr_r, eid_r, indices_r, n_k);
  const auto ppc = get_plan(col, indptr_c, eid_c, indices_c, n_q);
  const auto &pr = *ppr, &pc = *ppc;
  int64_t nbytes = 0;
  if (b) {
    check_attn_bias(fn, *b, Q, e, h);
    check(graphop_attention_bias_workspace_bytes(dtype_code(Q), 1, e, n_q, n_k, h, d, pr.plan, pc.plan, stream_of(Q),
                                                 need_db ? 1 : 0, &nbytes));
  } else {
    check((drop ? graphop_attention_dropout_workspace_bytes : graphop_attention_workspace_bytes)(
        dtype_code(Q), 1, e, n_q, n_k, h, d, pr.plan, pc.plan, stream_of(Q), &nbytes));
  }
  auto ws = at::empty({std::max<int64_t>(nbytes, 1)}, Q.options().dtype(at::kByte));
  if (b) {
    // db[e] is written once per row-major slot: only a chunk list that leaves slots out needs the zeros
    auto db = !need_db ? at::empty({0}, b->options()) : (pr.info.full_coverage ? at::empty_like(*b) : at::zeros_like(*b));
    check(graphop_attention_bias_backward(
        dtype_code(Q), ip(row), ip(indptr_r), ip(eid_r), ip(indices_r), ip(col), ip(indptr_c), ip(eid_c), ip(indices_c),
        vp(Q), vp(K), vp(V), vp(*b), vp(o), vp(stats), vp(dO), vp(dQ), vp(dK), vp(dV), need_db ? vp(db) : nullptr,
        row.size(0), col.size(0), e, n_q, n_k, h, d, ws.data_ptr(), nbytes, pr.plan, pc.plan, stream_of(Q), drop->p,
        drop->seed, drop->offset, head0));
    return {dQ, dK, dV, db};
  }
  if (drop)
    check(graphop_attention_dropout_backward(
        dtype_code(Q), ip(row), ip(indptr_r), ip(eid_r), ip(indices_r), ip(col), ip(indptr_c), ip(eid_c), ip(indices_c),
        vp(Q), vp(K), vp(V), vp(o), vp(stats), vp(dO), vp(dQ), vp(dK), vp(dV), row.size(0), col.size(0), e, n_q, n_k, h, d,
        ws.data_ptr(), nbytes, pr.plan, pc.plan, stream_of(Q), drop->p, drop->seed, drop->offset, head0));
  else
    check(graphop_attention_backward(dtype_code(Q), ip(row), ip(indptr_r), ip(eid_r), ip(indices_r), ip(col), ip(indptr_c),
                                     ip(eid_c), ip(indices_c), vp(Q), vp(K), vp(V), vp(o), vp(stats), vp(dO), vp(dQ),
                                     vp(dK), vp(dV), row.size(0), col.size(0), e, n_q, n_k, h, d, ws.data_ptr(), nbytes,
                                     pr.plan, pc.plan, stream_of(Q)));
  return {dQ, dK, dV};
}

std::vector<at::Tensor> attention_backward(const at::Tensor& row, const at::Tensor& indptr_r, const at::Tensor& eid_r,
                                           const at::Tensor& indices_r, const at::Tensor& col,
                                           const at::Tensor& indptr_c, const at::Tensor& eid_c,
                                           const at::Tensor& indices_c, const at::Tensor& Q, const at::Tensor& K,
                                           const at::Tensor& V, const at::Tensor& o, const at::Tensor& stats,
                                           const at::Tensor& dO) {
  return attention_backward_impl("attention_backward", row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c,
                                 Q, K, V, o, stats, dO, nullptr, 0);
}

std::vector<at::Tensor> attention_dropout_backward(const at::Tensor& row, const at::Tensor& indptr_r,
                                                   const at::Tensor& eid_r, const at::Tensor& indices_r,
                                                   const at::Tensor& col, const at::Tensor& indptr_c,
                                                   const at::Tensor& eid_c, const at::Tensor& indices_c,
                                                   const at::Tensor& Q, const at::Tensor& K, const at::Tensor& V,
                                                   const at::Tensor& o, const at::Tensor& stats, const at::Tensor& dO,
                                                   double p, int64_t seed, int64_t offset, int64_t head0) {
  const char* fn = "attention_dropout_backward";
  const DropSpec drop = drop_spec(fn, p, seed, offset);
  return attention_backward_impl(fn, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, o, stats,
                                 dO, &drop, head0_checked(fn, head0));
}

std::vector<at::Tensor> attention_bias_backward(const at::Tensor& row, const at::Tensor& indptr_r,
                                                const at::Tensor& eid_r, const at::Tensor& indices_r,
                                                const at::Tensor& col, const at::Tensor& indptr_c,
                                                const at::Tensor& eid_c, const at::Tensor& indices_c, const at::Tensor& Q,
                                                const at::Tensor& K, const at::Tensor& V, const at::Tensor& b,
                                                const at::Tensor& o, const at::Tensor& stats, const at::Tensor& dO,
                                                double p, int64_t seed, int64_t offset, int64_t head0, bool need_db) {
  const char* fn = "attention_bias_backward";
  const DropSpec drop = drop_spec(fn, p, seed, offset);
  return attention_backward_impl(fn, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, Q, K, V, o, stats,
                                 dO, &drop, head0_checked(fn, head0), &b, need_db);
}

// ---- edge features of the fused attention step (include/graphop_hip.h: graphop_attention_edge_*) ------------------------
// xe: a contiguous device tensor (n_edges, d) for 2-D Q / K / V, else (n_edges, h, d), in Q's dtype
void check_attn_edge_rows(const char* fn, const at::Tensor& xe, const at::Tensor& Q, int64_t e) {
  CHECK_SAME_DTYPE(Q, xe);
  TORCH_CHECK(xe.dim() == Q.dim() && xe.size(0) == e && xe.sizes().slice(1) == Q.sizes().slice(1),
              fn, ": xe must be (n_edges, d) for 2-D Q / K / V, else (n_edges, h, d) with n_edges = ", e, ", got xe ",
              xe.sizes(), ", Q ", Q.sizes());
  CHECK_CONTIGUOUS(xe); CHECK_CUDA(xe);
}

// edge-type embeddings (include/graphop_hip.h: graphop_attention_etype_*), the edge rows being R[etype[e]]:
// R: a contiguous device tensor (n_types, d) for 2-D Q / K / V, else (n_types, h, d), in Q's dtype, n_types >= 1 unless
// the graph has no edge; etype: a contiguous device int32 tensor (n_edges).  The values of etype are not looked at (that
// would synchronise): the kernels clamp them.
void check_attn_etype_table(const char* fn, const at::Tensor& R, const at::Tensor& etype, const at::Tensor& Q, int64_t e) {
  CHECK_SAME_DTYPE(Q, R);
  TORCH_CHECK(R.dim() == Q.dim() && R.sizes().slice(1) == Q.sizes().slice(1),
              fn, ": R must be (n_types, d) for 2-D Q / K / V, else (n_types, h, d), got R ", R.sizes(), ", Q ", Q.sizes());
  TORCH_CHECK(R.size(0) > 0 || e == 0, fn, ": R must hold at least one type (n_edges = ", e, ")");
  TORCH_CHECK(etype.scalar_type() == at::kInt, fn, ": etype must be torch.int32, got ", etype.scalar_type());
  TORCH_CHECK(etype.dim() == 1 && etype.size(0) == e,
              fn, ": etype must be (n_edges) with n_edges = ", e, ", got ", etype.sizes());
  CHECK_CONTIGUOUS(R); CHECK_CUDA(R);
  CHECK_CONTIGUOUS(etype); CHECK_CUDA(etype);
}

// an edge-type score bias (include/graphop_hip.h: graphop_attention_tbias_*), the score term being B[etype[e], k]:
// B: a contiguous device tensor (n_types) for 2-D Q / K / V, else (n_types, h), in Q's dtype, n_types >= 1 unless the
// graph has no edge; etype: a contiguous device int32 tensor (n_edges).  The values of etype are not looked at (that
// would synchronise): the kernels clamp them.
void check_attn_tbias_table(const char* fn, const at::Tensor& B, const at::Tensor& etype, const at::Tensor& Q, int64_t e) {
  CHECK_SAME_DTYPE(Q, B);
  TORCH_CHECK(B.dim() == Q.dim() - 1 && B.sizes().slice(1) == Q.sizes().slice(1, Q.dim() - 2),
              fn, ": B must be (n_types) for 2-D Q / K / V, else (n_types, h), got B ", B.sizes(), ", Q ", Q.sizes());
  TORCH_CHECK(B.size(0) > 0 || e == 0, fn, ": B must hold at least one type (n_edges = ", e, ")");
  TORCH_CHECK(etype.scalar_type() == at::kInt, fn, ": etype must be torch.int32, got ", etype.scalar_type());
  TORCH_CHECK(etype.dim() == 1 && etype.size(0) == e,
              fn, ": etype must be (n_edges) with n_edges = ", e, ", got ", etype.sizes());
  CHECK_CONTIGUOUS(B); CHECK_CUDA(B);
  CHECK_CONTIGUOUS(etype); CHECK_CUDA(etype);
}

// The entry points of the two ops that take a table and the types: one argument list, so one pointer type each
struct AttnTableAbi {
  decltype(&graphop_attention_etype_workspace_bytes) query;
  decltype(&graphop_attention_etype_forward) forward;
  decltype(&graphop_attention_etype_backward) backward;
  decltype(&check_attn_etype_table) check;
};
const AttnTableAbi kAttnEtypeAbi = {graphop_attention_etype_workspace_bytes, graphop_attention_etype_forward,
                                    graphop_attention_etype_backward, check_attn_etype_table};
const AttnTableAbi kAttnTbiasAbi = {graphop_attention_tbias_workspace_bytes, graphop_attention_tbias_forward,
                                    graphop_attention_tbias_backward, check_attn_tbias_table};

// The forward of the ops with an edge row in key and value and of the op with an edge-type score bias, as `fn`.
// etype == nullptr: rows is xe (graphop_attention_edge_forward); else rows is the table of `abi`: R
// (graphop_attention_etype_forward) or B (graphop_attention_tbias_forward).
std::vector<at::Tensor> attention_edge_forward_impl(const char* fn, const at::Tensor& row, const at::Tensor& indptr,
                                                    const at::Tensor& eid, const at::Tensor& indices, const at::Tensor& Q,
                                                    const at::Tensor& K, const at::Tensor& V, const at::Tensor& rows,
                                                    const at::Tensor* etype, double p, int64_t seed, int64_t offset,
                                                    int64_t head0, const AttnTableAbi& abi = kAttnEtypeAbi) {
  const DropSpec drop = drop_spec(fn, p, seed, offset);
  head0_checked(fn, head0);
  CHECK_CSR(row, indptr, eid, indices);
  CHECK_INPUT(Q); CHECK_INPUT(K); CHECK_INPUT(V);
  TORCH_CHECK(K.sizes() == V.sizes() && Q.sizes().slice(1) == K.sizes().slice(1),
              fn, ": Q (n_q,[h,]d), K and V (n_k,[h,]d) expected");
  CHECK_SAME_DTYPE(Q, K); CHECK_SAME_DTYPE(Q, V);
  const int64_t e = eid.size(0), d = Q.size(-1), h = Q.dim() == 2 ? 1 : Q.size(1), n_q = Q.size(0), n_k = K.size(0);
  if (etype) abi.check(fn, rows, *etype, Q, e);
  else check_attn_edge_rows(fn, rows, Q, e);
  const int64_t n_types = rows.size(0);
  DeviceGuard dg(Q);
  auto o = at::empty_like(Q);
  auto stats = at::empty({n_q, h, 2}, Q.options());
  const auto pp = get_plan(row, indptr, eid, indices, n_k);
  const auto& pl = *pp;
  int64_t nbytes = 0;
  check(etype ? abi.query(dtype_code(Q), 0, e, n_q, n_k, h, d, n_types, pl.plan, nullptr, stream_of(Q), &nbytes)
              : graphop_attention_edge_workspace_bytes(dtype_code(Q), 0, e, n_q, n_k, h, d, pl.plan, nullptr,
                                                       stream_of(Q), &nbytes));
  auto ws = at::empty({std::max<int64_t>(nbytes, 1)}, Q.options().dtype(at::kByte));
  if (etype)
    check(abi.forward(dtype_code(Q), ip(row), ip(indptr), ip(eid), ip(indices), vp(Q), vp(K), vp(V), vp(rows),
                      etype->data_ptr<int32_t>(), vp(o), vp(stats), row.size(0), e, n_q, n_k, h, d, n_types, ws.data_ptr(),
                      nbytes, pl.plan, stream_of(Q), drop.p, drop.seed, drop.offset, head0));
  else
    check(graphop_attention_edge_forward(dtype_code(Q), ip(row), ip(indptr), ip(eid), ip(indices), vp(Q), vp(K), vp(V),
                                         vp(rows), vp(o), vp(stats), row.size(0), e, n_q, n_k, h, d, ws.data_ptr(), nbytes,
                                         pl.plan, stream_of(Q), drop.p, drop.seed, drop.offset, head0));
  return {o, stats};
}

std::vector<at::Tensor> attention_edge_forward(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                                               const at::Tensor& indices, const at::Tensor& Q, const at::Tensor& K,
                                               const at::Tensor& V, const at::Tensor& xe, double p, int64_t seed,
                                               int64_t offset, int64_t head0) {
  return attention_edge_forward_impl("attention_edge_forward", row, indptr, eid, indices, Q, K, V, xe, nullptr, p, seed,
                                     offset, head0);
}

std::vector<at::Tensor> attention_etype_forward(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                                                const at::Tensor& indices, const at::Tensor& Q, const at::Tensor& K,
                                                const at::Tensor& V, const at::Tensor& R, const at::Tensor& etype,
                                                double p, int64_t seed, int64_t offset, int64_t head0) {
  return attention_edge_forward_impl("attention_etype_forward", row, indptr, eid, indices, Q, K, V, R, &etype, p, seed,
                                     offset, head0);
}

// The backward of the same two ops; the fourth tensor is the gradient of rows, empty with need_dx == false
std::vector<at::Tensor> attention_edge_backward_impl(const char* fn, const at::Tensor& row, const at::Tensor& indptr_r,
                                                     const at::Tensor& eid_r, const at::Tensor& indices_r,
                                                     const at::Tensor& col, const at::Tensor& indptr_c,
                                                     const at::Tensor& eid_c, const at::Tensor& indices_c,
                                                     const at::Tensor& Q, const at::Tensor& K, const at::Tensor& V,
                                                     const at::Tensor& rows, const at::Tensor* etype, const at::Tensor& o,
                                                     const at::Tensor& stats, const at::Tensor& dO_, double p,
                                                     int64_t seed, int64_t offset, int64_t head0, bool need_dx,
                                                     const AttnTableAbi& abi = kAttnEtypeAbi) {
  const DropSpec drop = drop_spec(fn, p, seed, offset);
  head0_checked(fn, head0);
  CHECK_CSR(row, indptr_r, eid_r, indices_r);
  CHECK_CSR(col, indptr_c, eid_c, indices_c);
  CHECK_INPUT(Q); CHECK_INPUT(K); CHECK_INPUT(V); CHECK_INPUT(o); CHECK_INPUT(stats);
  CHECK_CUDA(dO_);
  const at::Tensor dO = dO_.contiguous();
  CHECK_SAME_DTYPE(Q, K); CHECK_SAME_DTYPE(Q, V); CHECK_SAME_DTYPE(Q, o); CHECK_SAME_DTYPE(Q, stats); CHECK_SAME_DTYPE(Q, dO);
  TORCH_CHECK(K.sizes() == V.sizes() && Q.sizes().slice(1) == K.sizes().slice(1),
              fn, ": Q (n_q,[h,]d), K and V (n_k,[h,]d) expected");
  const int64_t e = eid_r.size(0), d = Q.size(-1), h = Q.dim() == 2 ? 1 : Q.size(1), n_q = Q.size(0), n_k = K.size(0);
  TORCH_CHECK(o.sizes() == Q.sizes() && dO.sizes() == Q.sizes() && stats.numel() == n_q * h * 2,
              fn, ": o, dO must match Q and stats must be (n_q, h, 2)");
  if (etype) abi.check(fn, rows, *etype, Q, e);
  else check_attn_edge_rows(fn, rows, Q, e);
  const int64_t n_types = rows.size(0);
  DeviceGuard dg(Q);
  auto dQ = at::empty_like(Q), dK = at::empty_like(K), dV = at::empty_like(V);
  const auto ppr = get_plan(row, indptr_r, eid_r, indices_r, n_k);
  const auto ppc = get_plan(col, indptr_c, eid_c, indices_c, n_q);
  const auto &pr = *ppr, &pc = *ppc;
  int64_t nbytes = 0;
  check(etype ? abi.query(dtype_code(Q), 1, e, n_q, n_k, h, d, n_types, pr.plan, pc.plan, stream_of(Q), &nbytes)
              : graphop_attention_edge_workspace_bytes(dtype_code(Q), 1, e, n_q, n_k, h, d, pr.plan, pc.plan,
                                                       stream_of(Q), &nbytes));
  auto ws = at::empty({std::max<int64_t>(nbytes, 1)}, Q.options().dtype(at::kByte));
  // dR, dB: the call fills it.  dxe[e] is written once per row-major slot: only a chunk list that leaves slots out needs
  // the zeros
  auto dx = !need_dx ? at::empty({0}, rows.options())
                     : (etype || pr.info.full_coverage ? at::empty_like(rows) : at::zeros_like(rows));
  if (etype)
    check(abi.backward(
        dtype_code(Q), ip(row), ip(indptr_r), ip(eid_r), ip(indices_r), ip(col), ip(indptr_c), ip(eid_c), ip(indices_c),
        vp(Q), vp(K), vp(V), vp(rows), etype->data_ptr<int32_t>(), vp(o), vp(stats), vp(dO), vp(dQ), vp(dK), vp(dV),
        need_dx ? vp(dx) : nullptr, row.size(0), col.size(0), e, n_q, n_k, h, d, n_types, ws.data_ptr(), nbytes, pr.plan,
        pc.plan, stream_of(Q), drop.p, drop.seed, drop.offset, head0));
  else
    check(graphop_attention_edge_backward(
        dtype_code(Q), ip(row), ip(indptr_r), ip(eid_r), ip(indices_r), ip(col), ip(indptr_c), ip(eid_c), ip(indices_c),
        vp(Q), vp(K), vp(V), vp(rows), vp(o), vp(stats), vp(dO), vp(dQ), vp(dK), vp(dV), need_dx ? vp(dx) : nullptr,
        row.size(0), col.size(0), e, n_q, n_k, h, d, ws.data_ptr(), nbytes, pr.plan, pc.plan, stream_of(Q), drop.p,
        drop.seed, drop.offset, head0));
  return {dQ, dK, dV, dx};
}

std::vector<at::Tensor> attention_edge_backward(const at::Tensor& row, const at::Tensor& indptr_r,
                                                const at::Tensor& eid_r, const at::Tensor& indices_r,
                                                const at::Tensor& col, const at::Tensor& indptr_c,
                                                const at::Tensor& eid_c, const at::Tensor& indices_c, const at::Tensor& Q,
                                                const at::Tensor& K, const at::Tensor& V, const at::Tensor& xe,
                                                const at::Tensor& o, const at::Tensor& stats, const at::Tensor& dO,
                                                double p, int64_t seed, int64_t offset, int64_t head0, bool need_dxe) {
  return attention_edge_backward_impl("attention_edge_backward", row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c,
                                      indices_c, Q, K, V, xe, nullptr, o, stats, dO, p, seed, offset, head0, need_dxe);
}

std::vector<at::Tensor> attention_etype_backward(const at::Tensor& row, const at::Tensor& indptr_r,
                                                 const at::Tensor& eid_r, const at::Tensor& indices_r,
                                                 const at::Tensor& col, const at::Tensor& indptr_c,
                                                 const at::Tensor& eid_c, const at::Tensor& indices_c, const at::Tensor& Q,
                                                 const at::Tensor& K, const at::Tensor& V, const at::Tensor& R,
                                                 const at::Tensor& etype, const at::Tensor& o, const at::Tensor& stats,
                                                 const at::Tensor& dO, double p, int64_t seed, int64_t offset,
                                                 int64_t head0, bool need_dR) {
  return attention_edge_backward_impl("attention_etype_backward", row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c,
                                      indices_c, Q, K, V, R, &etype, o, stats, dO, p, seed, offset, head0, need_dR);
}

std::vector<at::Tensor> attention_tbias_forward(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                                                const at::Tensor& indices, const at::Tensor& Q, const at::Tensor& K,
                                                const at::Tensor& V, const at::Tensor& B, const at::Tensor& etype,
                                                double p, int64_t seed, int64_t offset, int64_t head0) {
  return attention_edge_forward_impl("attention_tbias_forward", row, indptr, eid, indices, Q, K, V, B, &etype, p, seed,
                                     offset, head0, kAttnTbiasAbi);
}

std::vector<at::Tensor> attention_tbias_backward(const at::Tensor& row, const at::Tensor& indptr_r,
                                                 const at::Tensor& eid_r, const at::Tensor& indices_r,
                                                 const at::Tensor& col, const at::Tensor& indptr_c,
                                                 const at::Tensor& eid_c, const at::Tensor& indices_c, const at::Tensor& Q,
                                                 const at::Tensor& K, const at::Tensor& V, const at::Tensor& B,
                                                 const at::Tensor& etype, const at::Tensor& o, const at::Tensor& stats,
                                                 const at::Tensor& dO, double p, int64_t seed, int64_t offset,
                                                 int64_t head0, bool need_dB) {
  return attention_edge_backward_impl("attention_tbias_backward", row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c,
                                      indices_c, Q, K, V, B, &etype, o, stats, dO, p, seed, offset, head0, need_dB,
                                      kAttnTbiasAbi);
}

// ---- the weights of the fused attention ops from their row statistics (include/graphop_hip.h: graphop_attention_weights)
at::Tensor attention_weights(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                             const at::Tensor& indices, const at::Tensor& Q, const at::Tensor& K, const at::Tensor& stats,
                             const c10::optional<at::Tensor>& b, const c10::optional<at::Tensor>& xe) {
  const char* fn = "attention_weights";
  CHECK_CSR(row, indptr, eid, indices);
  CHECK_INPUT(Q); CHECK_INPUT(K); CHECK_INPUT(stats);
  if (b) check_attn_bias_input(*b);
  TORCH_CHECK(!(b && xe), fn, ": at most one of b and xe may be given");
  CHECK_SAME_DTYPE(Q, K); CHECK_SAME_DTYPE(Q, stats);
  TORCH_CHECK((Q.dim() == 2 || Q.dim() == 3) && Q.sizes().slice(1) == K.sizes().slice(1),
              fn, ": Q (n_q,[h,]d) and K (n_k,[h,]d) expected");
  const int64_t e = eid.size(0), d = Q.size(-1), h = Q.dim() == 2 ? 1 : Q.size(1), n_q = Q.size(0), n_k = K.size(0);
  TORCH_CHECK(stats.dim() == 3 && stats.size(0) == n_q && stats.size(1) == h && stats.size(2) == 2,
              fn, ": stats must be (n_q, h, 2) = (", n_q, ", ", h, ", 2), got ", stats.sizes());
  if (b) check_attn_bias(fn, *b, Q, e, h);
  if (xe) check_attn_edge_rows(fn, *xe, Q, e);
  DeviceGuard dg(Q);
  const auto pp = get_plan(row, indptr, eid, indices, n_k);
  const auto& pl = *pp;
  // a[e] is written once per row-major slot: only a chunk list that leaves slots out needs the zeros
  const std::vector<int64_t> shape = Q.dim() == 2 ? std::vector<int64_t>{e} : std::vector<int64_t>{e, h};
  auto a = pl.info.full_coverage ? at::empty(shape, Q.options()) : at::zeros(shape, Q.options());
  check(graphop_attention_weights(dtype_code(Q), ip(row), ip(indptr), ip(eid), ip(indices), vp(Q), vp(K), vp(stats),
                                  b ? vp(*b) : nullptr, xe ? vp(*xe) : nullptr, vp(a), row.size(0), e, n_q, n_k, h, d,
                                  pl.plan, stream_of(Q)));
  return a;
}

// ---- the extra GAT score op (include/graphop_hip.h: graphop_gat_scores_*) ---------------------------------
int64_t gat_heads(const at::Tensor& el, const at::Tensor& er, const char* fn) {
  CHECK_SAME_DTYPE(el, er);
  TORCH_CHECK((el.dim() == 1 || el.dim() == 2) && er.dim() == el.dim() && (el.dim() == 1 || el.size(1) == er.size(1)),
              fn, ": el (n_src[, h]) and er (n_dst[, h]) must have the same h, got ", el.sizes(), " and ", er.sizes());
  return el.dim() == 1 ? 1 : el.size(1);
}

at::Tensor gat_scores_forward(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                              const at::Tensor& indices, const at::Tensor& el, const at::Tensor& er,
                              double negative_slope) {
  CHECK_CSR(row, indptr, eid, indices);
  CHECK_INPUT(el); CHECK_INPUT(er);
  const int64_t h = gat_heads(el, er, "gat_scores_forward");
  DeviceGuard dg(el);
  const int64_t e = eid.size(0);
  auto y = edge_out(el, e, h);
  const auto pp = get_plan(row, indptr, eid, indices, er.size(0));
  const auto& p = *pp;
  check(graphop_gat_scores_forward(dtype_code(el), ip(row), ip(indptr), ip(eid), ip(indices), vp(el), vp(er), vp(y),
                                   row.size(0), e, el.size(0), er.size(0), h, negative_slope, p.plan, stream_of(el)));
  return y;
}

std::vector<at::Tensor> gat_scores_backward(const at::Tensor& row, const at::Tensor& indptr_r, const at::Tensor& eid_r,
                                            const at::Tensor& indices_r, const at::Tensor& col,
                                            const at::Tensor& indptr_c, const at::Tensor& eid_c,
                                            const at::Tensor& indices_c, const at::Tensor& el, const at::Tensor& er,
                                            const at::Tensor& dy_, double negative_slope) {
  CHECK_CSR(row, indptr_r, eid_r, indices_r);
  CHECK_CSR(col, indptr_c, eid_c, indices_c);
  CHECK_INPUT(el); CHECK_INPUT(er);
  CHECK_CUDA(dy_);
  const at::Tensor dy = dy_.contiguous();
  const int64_t h = gat_heads(el, er, "gat_scores_backward");
  CHECK_SAME_DTYPE(el, dy);
  const int64_t e = eid_r.size(0);
  TORCH_CHECK(dy.numel() == e * h, "gat_scores_backward: dy must hold (n_edges, h) = (", e, ", ", h, ") values, got ",
              dy.sizes());
  DeviceGuard dg(el);
  auto d_el = at::empty_like(el), d_er = at::empty_like(er);
  const auto ppr = get_plan(row, indptr_r, eid_r, indices_r, er.size(0));
  const auto ppc = get_plan(col, indptr_c, eid_c, indices_c, el.size(0));
  const auto &pr = *ppr, &pc = *ppc;
  check(graphop_gat_scores_backward(dtype_code(el), ip(row), ip(indptr_r), ip(eid_r), ip(indices_r), ip(col),
                                    ip(indptr_c), ip(eid_c), ip(indices_c), vp(el), vp(er), vp(dy), vp(d_el), vp(d_er),
                                    row.size(0), col.size(0), e, el.size(0), er.size(0), h, negative_slope, pr.plan,
                                    pc.plan, stream_of(el)));
  return {d_el, d_er};
}

// ---- the extra GATv2 score op (include/graphop_hip.h: graphop_gatv2_scores_*) ------------------------------------
std::pair<int64_t, int64_t> gatv2_shapes(const at::Tensor& xl, const at::Tensor& xr, const at::Tensor& att,
                                         const char* fn) {
  CHECK_SAME_DTYPE(xl, xr);
  CHECK_SAME_DTYPE(xl, att);
  TORCH_CHECK((xl.dim() == 2 || xl.dim() == 3) && xr.dim() == xl.dim() && (xl.dim() == 2 || xl.size(1) == xr.size(1)),
              fn, ": xl (n_src[, h], d) and xr (n_dst[, h], d) must have the same h, got ", xl.sizes(), " and ",
              xr.sizes());
  TORCH_CHECK(xl.size(-1) == xr.size(-1), fn, ": xl and xr must have the same d, got ", xl.sizes(), " and ", xr.sizes());
  TORCH_CHECK(att.sizes() == xl.sizes().slice(1), fn, ": att must be ", xl.sizes().slice(1),
              " (the same h and the same d as xl), got ", att.sizes());
  return {xl.dim() == 2 ? 1 : xl.size(1), xl.size(-1)};
}

at::Tensor gatv2_scores_forward(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                                const at::Tensor& indices, const at::Tensor& xl, const at::Tensor& xr,
                                const at::Tensor& att, double negative_slope) {
  CHECK_CSR(row, indptr, eid, indices);
  CHECK_INPUT(xl); CHECK_INPUT(xr); CHECK_INPUT(att);
  const auto hd = gatv2_shapes(xl, xr, att, "gatv2_scores_forward");
  const int64_t h = hd.first, d = hd.second;
  DeviceGuard dg(xl);
  const int64_t e = eid.size(0);
  auto y = xl.dim() == 2 ? at::empty({e}, xl.options()) : at::empty({e, h}, xl.options());
  const auto pp = get_plan(row, indptr, eid, indices, xr.size(0));
  const auto& p = *pp;
  check(graphop_gatv2_scores_forward(dtype_code(xl), ip(row), ip(indptr), ip(eid), ip(indices), vp(xl), vp(xr), vp(att),
                                     vp(y), row.size(0), e, xl.size(0), xr.size(0), h, d, negative_slope, p.plan,
                                     stream_of(xl)));
  return y;
}

std::vector<at::Tensor> gatv2_scores_backward(const at::Tensor& row, const at::Tensor& indptr_r,
                                              const at::Tensor& eid_r, const at::Tensor& indices_r,
                                              const at::Tensor& col, const at::Tensor& indptr_c,
                                              const at::Tensor& eid_c, const at::Tensor& indices_c,
                                              const at::Tensor& xl, const at::Tensor& xr, const at::Tensor& att,
                                              const at::Tensor& dy_, double negative_slope) {
  CHECK_CSR(row, indptr_r, eid_r, indices_r);
  CHECK_CSR(col, indptr_c, eid_c, indices_c);
  CHECK_INPUT(xl); CHECK_INPUT(xr); CHECK_INPUT(att);
  CHECK_CUDA(dy_);
  const at::Tensor dy = dy_.contiguous();
  const auto hd = gatv2_shapes(xl, xr, att, "gatv2_scores_backward");
  const int64_t h = hd.first, d = hd.second;
  CHECK_SAME_DTYPE(xl, dy);
  const int64_t e = eid_r.size(0);
  TORCH_CHECK(dy.numel() == e * h, "gatv2_scores_backward: dy must hold (n_edges, h) = (", e, ", ", h,
              ") values, got ", dy.sizes());
  DeviceGuard dg(xl);
  auto dxl = at::empty_like(xl), dxr = at::empty_like(xr), datt = at::empty_like(att);
  auto ws = at::empty({std::max<int64_t>(gatv2_row_pass_values(row.size(0), h, d), 1)}, xl.options());
  const auto ppr = get_plan(row, indptr_r, eid_r, indices_r, xr.size(0));
  const auto ppc = get_plan(col, indptr_c, eid_c, indices_c, xl.size(0));
  const auto &pr = *ppr, &pc = *ppc;
  check(graphop_gatv2_scores_backward(dtype_code(xl), ip(row), ip(indptr_r), ip(eid_r), ip(indices_r), ip(col),
                                      ip(indptr_c), ip(eid_c), ip(indices_c), vp(xl), vp(xr), vp(att), vp(dy), vp(dxl),
                                      vp(dxr), vp(datt), vp(ws), ws.numel() * ws.element_size(), row.size(0),
                                      col.size(0), e, xl.size(0), xr.size(0), h, d, negative_slope, pr.plan, pc.plan,
                                      stream_of(xl)));
  return {dxl, dxr, datt};
}

// ---- the fused GATv2 attention op (include/graphop_hip.h: graphop_gatv2_attention_*) ------------------------------
// the edge rows of graphop_gatv2_edge_attention_*: (n_edges, d) for 2-D xl / xr, else (n_edges, h, d), in xl's dtype
void gatv2_edge_rows(const at::Tensor& xl, const at::Tensor& xe, int64_t n_edges, int64_t h, int64_t d,
                     const char* fn) {
  CHECK_INPUT(xe);
  CHECK_SAME_DTYPE(xl, xe);
  const bool tail = xl.dim() == 2 ? (xe.dim() == 2 && xe.size(1) == d)
                                  : (xe.dim() == 3 && xe.size(1) == h && xe.size(2) == d);
  if (tail) CHECK_EDGE_ROWS(xe, n_edges);
  TORCH_CHECK(tail && xe.size(0) == n_edges, fn, ": xe must be (n_edges, d) for 2-D xl / xr, else (n_edges, h, d) with "
              "n_edges = ", n_edges, ", h = ", h, " and d = ", d, ", got xe ", xe.sizes(), ", xl ", xl.sizes());
}

// drop == nullptr: graphop_gatv2_attention_forward, else its dropout form or, with the edge rows xe (which need drop),
// graphop_gatv2_edge_attention_forward, as `fn`
std::vector<at::Tensor> gatv2_attention_forward_impl(const char* fn, const at::Tensor& row, const at::Tensor& indptr,
                                                     const at::Tensor& eid, const at::Tensor& indices,
                                                     const at::Tensor& xl, const at::Tensor& xr, const at::Tensor& att,
                                                     double negative_slope, const DropSpec* drop,
                                                     const at::Tensor* xe = nullptr) {
  CHECK_CSR(row, indptr, eid, indices);
  CHECK_INPUT(xl); CHECK_INPUT(xr); CHECK_INPUT(att);
  const auto hd = gatv2_shapes(xl, xr, att, fn);
  const int64_t h = hd.first, d = hd.second;
  const int64_t e = eid.size(0), n_l = xl.size(0);
  if (xe) gatv2_edge_rows(xl, *xe, e, h, d, fn);
  DeviceGuard dg(xl);
  auto o = at::empty_like(xl);
  auto stats = at::empty({n_l, h, 2}, xl.options());
  const auto pp = get_plan(row, indptr, eid, indices, xr.size(0));
  const auto& p = *pp;
  if (xe)
    check(graphop_gatv2_edge_attention_forward(dtype_code(xl), ip(row), ip(indptr), ip(eid), ip(indices), vp(xl), vp(xr),
                                               vp(*xe), vp(att), vp(o), vp(stats), row.size(0), e, n_l, xr.size(0), h, d,
                                               negative_slope, drop->p, drop->seed, drop->offset, p.plan,
                                               stream_of(xl)));
  else if (drop)
    check(graphop_gatv2_attention_dropout_forward(dtype_code(xl), ip(row), ip(indptr), ip(eid), ip(indices), vp(xl),
                                                  vp(xr), vp(att), vp(o), vp(stats), row.size(0), e, n_l, xr.size(0), h,
                                                  d, negative_slope, drop->p, drop->seed, drop->offset, p.plan,
                                                  stream_of(xl)));
  else
    check(graphop_gatv2_attention_forward(dtype_code(xl), ip(row), ip(indptr), ip(eid), ip(indices), vp(xl), vp(xr),
                                          vp(att), vp(o), vp(stats), row.size(0), e, n_l, xr.size(0), h, d,
                                          negative_slope, p.plan, stream_of(xl)));
  return {o, stats};
}

std::vector<at::Tensor> gatv2_attention_forward(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                                                const at::Tensor& indices, const at::Tensor& xl, const at::Tensor& xr,
                                                const at::Tensor& att, double negative_slope) {
  return gatv2_attention_forward_impl("gatv2_attention_forward", row, indptr, eid, indices, xl, xr, att, negative_slope,
                                      nullptr);
}

std::vector<at::Tensor> gatv2_attention_dropout_forward(const at::Tensor& row, const at::Tensor& indptr,
                                                        const at::Tensor& eid, const at::Tensor& indices,
                                                        const at::Tensor& xl, const at::Tensor& xr,
                                                        const at::Tensor& att, double negative_slope, double p,
                                                        int64_t seed, int64_t offset,
                                                        const c10::optional<at::Tensor>& xe) {
  const char* fn = "gatv2_attention_dropout_forward";
  const DropSpec drop = drop_spec(fn, p, seed, offset);
  return gatv2_attention_forward_impl(fn, row, indptr, eid, indices, xl, xr, att, negative_slope, &drop,
                                      xe.has_value() ? &*xe : nullptr);
}

std::vector<at::Tensor> gatv2_attention_backward_impl(const char* fn, const at::Tensor& row,
                                                      const at::Tensor& indptr_r, const at::Tensor& eid_r,
                                                      const at::Tensor& indices_r, const at::Tensor& col,
                                                      const at::Tensor& indptr_c, const at::Tensor& eid_c,
                                                      const at::Tensor& indices_c, const at::Tensor& xl,
                                                      const at::Tensor& xr, const at::Tensor& att, const at::Tensor& o,
                                                      const at::Tensor& stats, const at::Tensor& dO_,
                                                      double negative_slope, const DropSpec* drop,
                                                      const at::Tensor* xe = nullptr, bool need_dxe = true) {
  CHECK_CSR(row, indptr_r, eid_r, indices_r);
  CHECK_CSR(col, indptr_c, eid_c, indices_c);
  CHECK_INPUT(xl); CHECK_INPUT(xr); CHECK_INPUT(att); CHECK_INPUT(o); CHECK_INPUT(stats);
  CHECK_CUDA(dO_);
  const auto hd = gatv2_shapes(xl, xr, att, fn);
  const int64_t h = hd.first, d = hd.second;
  const int64_t e = eid_r.size(0), n_l = xl.size(0);
  if (xe) gatv2_edge_rows(xl, *xe, e, h, d, fn);
  CHECK_SAME_DTYPE(xl, o); CHECK_SAME_DTYPE(xl, stats); CHECK_SAME_DTYPE(xl, dO_);
  const at::Tensor dO = saved_checked(fn, xl.sizes(), n_l, h, o, stats, dO_);
  DeviceGuard dg(xl);
  auto dxl = at::empty_like(xl), dxr = at::empty_like(xr), datt = at::empty_like(att);
  // the workspace minimum of include/graphop_hip.h: (m, 1 / l, D, 0) per (node, head), then the row-pass partials
  const int64_t ws_values = n_l * h * 4 + gatv2_row_pass_values(row.size(0), h, d);
  auto ws = at::empty({std::max<int64_t>(ws_values, 1)}, xl.options());
  const auto ppr = get_plan(row, indptr_r, eid_r, indices_r, xr.size(0));
  const auto ppc = get_plan(col, indptr_c, eid_c, indices_c, n_l);
  const auto &pr = *ppr, &pc = *ppc;
  if (xe) {
    auto dxe = need_dxe ? at::empty_like(*xe) : at::empty({0}, xe->options());   // the only edge-sized tensor made
    check(graphop_gatv2_edge_attention_backward(
        dtype_code(xl), ip(row), ip(indptr_r), ip(eid_r), ip(indices_r), ip(col), ip(indptr_c), ip(eid_c),
        ip(indices_c), vp(xl), vp(xr), vp(*xe), vp(att), vp(o), vp(stats), vp(dO), vp(dxl), vp(dxr),
        need_dxe ? vp(dxe) : nullptr, vp(datt), vp(ws), ws.numel() * ws.element_size(), row.size(0), col.size(0), e,
        n_l, xr.size(0), h, d, negative_slope, drop->p, drop->seed, drop->offset, pr.plan, pc.plan, stream_of(xl)));
    return {dxl, dxr, datt, dxe};
  }
  if (drop)
    check(graphop_gatv2_attention_dropout_backward(
        dtype_code(xl), ip(row), ip(indptr_r), ip(eid_r), ip(indices_r), ip(col), ip(indptr_c), ip(eid_c),
        ip(indices_c), vp(xl), vp(xr), vp(att), vp(o), vp(stats), vp(dO), vp(dxl), vp(dxr), vp(datt), vp(ws),
        ws.numel() * ws.element_size(), row.size(0), col.size(0), e, n_l, xr.size(0), h, d, negative_slope, drop->p,
        drop->seed, drop->offset, pr.plan, pc.plan, stream_of(xl)));
  else
    check(graphop_gatv2_attention_backward(dtype_code(xl), ip(row), ip(indptr_r), ip(eid_r), ip(indices_r), ip(col),
                                           ip(indptr_c), ip(eid_c), ip(indices_c), vp(xl), vp(xr), vp(att), vp(o),
                                           vp(stats), vp(dO), vp(dxl), vp(dxr), vp(datt), vp(ws),
                                           ws.numel() * ws.element_size(), row.size(0), col.size(0), e, n_l,
                                           xr.size(0), h, d, negative_slope, pr.plan, pc.plan, stream_of(xl)));
  return {dxl, dxr, datt};
}

std::vector<at::Tensor> gatv2_attention_backward(const at::Tensor& row, const at::Tensor& indptr_r,
                                                 const at::Tensor& eid_r, const at::Tensor& indices_r,
                                                 const at::Tensor& col, const at::Tensor& indptr_c,
                                                 const at::Tensor& eid_c, const at::Tensor& indices_c,
                                                 const at::Tensor& xl, const at::Tensor& xr, const at::Tensor& att,
                                                 const at::Tensor& o, const at::Tensor& stats, const at::Tensor& dO,
                                                 double negative_slope) {
  return gatv2_attention_backward_impl("gatv2_attention_backward", row, indptr_r, eid_r, indices_r, col, indptr_c,
                                       eid_c, indices_c, xl, xr, att, o, stats, dO, negative_slope, nullptr);
}

std::vector<at::Tensor> gatv2_attention_dropout_backward(const at::Tensor& row, const at::Tensor& indptr_r,
                                                         const at::Tensor& eid_r, const at::Tensor& indices_r,
                                                         const at::Tensor& col, const at::Tensor& indptr_c,
                                                         const at::Tensor& eid_c, const at::Tensor& indices_c,
                                                         const at::Tensor& xl, const at::Tensor& xr,
                                                         const at::Tensor& att, const at::Tensor& o,
                                                         const at::Tensor& stats, const at::Tensor& dO,
                                                         double negative_slope, double p, int64_t seed,
                                                         int64_t offset, const c10::optional<at::Tensor>& xe,
                                                         bool need_dxe) {
  const char* fn = "gatv2_attention_dropout_backward";
  const DropSpec drop = drop_spec(fn, p, seed, offset);
  return gatv2_attention_backward_impl(fn, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr,
                                       att, o, stats, dO, negative_slope, &drop, xe.has_value() ? &*xe : nullptr,
                                       need_dxe);
}

// ---- the fused GAT attention op (include/graphop_hip.h: graphop_gat_attention_*) -----------------------------------
std::pair<int64_t, int64_t> gat_attn_shapes(const at::Tensor& el, const at::Tensor& er, const at::Tensor& V,
                                            const char* fn) {
  const int64_t h = gat_heads(el, er, fn);
  CHECK_SAME_DTYPE(el, V);
  TORCH_CHECK(V.dim() == (el.dim() == 1 ? 2 : 3) && (V.dim() == 2 || V.size(1) == h) && V.size(0) == er.size(0), fn,
              ": V must be (n_dst, d) for 1-D el / er, else (n_dst, h, d) with the same h and n_dst as er, got V ",
              V.sizes(), ", er ", er.sizes());
  return {h, V.size(-1)};
}

// the edge term of graphop_gat_edge_attention_*: (n_edges) for 1-D el / er, else (n_edges, h), in el's dtype
void gat_edge_term(const at::Tensor& el, const at::Tensor& ee, int64_t n_edges, int64_t h, const char* fn) {
  CHECK_INPUT(ee);
  CHECK_SAME_DTYPE(el, ee);
  const bool ok = el.dim() == 1 ? (ee.dim() == 1 && ee.size(0) == n_edges)
                                : (ee.dim() == 2 && ee.size(0) == n_edges && ee.size(1) == h);
  TORCH_CHECK(ok, fn, ": ee must be (n_edges) for 1-D el / er, else (n_edges, h) with n_edges = ", n_edges, " and h = ",
              h, ", got ee ", ee.sizes(), ", el ", el.sizes());
}

// graphop_gat_attention_forward (drop == nullptr), its dropout form or, with the edge term ee (which needs drop),
// graphop_gat_edge_attention_forward, as `fn`
std::vector<at::Tensor> gat_attention_forward_impl(const char* fn, const at::Tensor& row, const at::Tensor& indptr,
                                                   const at::Tensor& eid, const at::Tensor& indices,
                                                   const at::Tensor& el, const at::Tensor& er, const at::Tensor& V,
                                                   double negative_slope, const DropSpec* drop,
                                                   const at::Tensor* ee = nullptr) {
  CHECK_CSR(row, indptr, eid, indices);
  CHECK_INPUT(el); CHECK_INPUT(er); CHECK_INPUT(V);
  const auto hd = gat_attn_shapes(el, er, V, fn);
  const int64_t h = hd.first, d = hd.second;
  const int64_t e = eid.size(0), n_l = el.size(0);
  if (ee) gat_edge_term(el, *ee, e, h, fn);
  DeviceGuard dg(el);
  auto o = at::empty(with_rows(V, n_l), V.options());
  auto stats = at::empty({n_l, h, 2}, el.options());
  const auto pp = get_plan(row, indptr, eid, indices, er.size(0));
  const auto& p = *pp;
  if (ee)
    check(graphop_gat_edge_attention_forward(dtype_code(el), ip(row), ip(indptr), ip(eid), ip(indices), vp(el), vp(er),
                                             vp(*ee), vp(V), vp(o), vp(stats), row.size(0), e, n_l, er.size(0), h, d,
                                             negative_slope, drop->p, drop->seed, drop->offset, p.plan, stream_of(el)));
  else if (drop)
    check(graphop_gat_attention_dropout_forward(dtype_code(el), ip(row), ip(indptr), ip(eid), ip(indices), vp(el),
                                                vp(er), vp(V), vp(o), vp(stats), row.size(0), e, n_l, er.size(0), h, d,
                                                negative_slope, drop->p, drop->seed, drop->offset, p.plan,
                                                stream_of(el)));
  else
    check(graphop_gat_attention_forward(dtype_code(el), ip(row), ip(indptr), ip(eid), ip(indices), vp(el), vp(er),
                                        vp(V), vp(o), vp(stats), row.size(0), e, n_l, er.size(0), h, d, negative_slope,
                                        p.plan, stream_of(el)));
  return {o, stats};
}

std::vector<at::Tensor> gat_attention_forward(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                                              const at::Tensor& indices, const at::Tensor& el, const at::Tensor& er,
                                              const at::Tensor& V, double negative_slope) {
  return gat_attention_forward_impl("gat_attention_forward", row, indptr, eid, indices, el, er, V, negative_slope,
                                    nullptr);
}

std::vector<at::Tensor> gat_attention_dropout_forward(const at::Tensor& row, const at::Tensor& indptr,
                                                      const at::Tensor& eid, const at::Tensor& indices,
                                                      const at::Tensor& el, const at::Tensor& er, const at::Tensor& V,
                                                      double negative_slope, double p, int64_t seed, int64_t offset) {
  const char* fn = "gat_attention_dropout_forward";
  const DropSpec drop = drop_spec(fn, p, seed, offset);
  return gat_attention_forward_impl(fn, row, indptr, eid, indices, el, er, V, negative_slope, &drop);
}

std::vector<at::Tensor> gat_edge_attention_forward(const at::Tensor& row, const at::Tensor& indptr,
                                                   const at::Tensor& eid, const at::Tensor& indices,
                                                   const at::Tensor& el, const at::Tensor& er, const at::Tensor& ee,
                                                   const at::Tensor& V, double negative_slope, double p, int64_t seed,
                                                   int64_t offset) {
  const char* fn = "gat_edge_attention_forward";
  const DropSpec drop = drop_spec(fn, p, seed, offset);
  return gat_attention_forward_impl(fn, row, indptr, eid, indices, el, er, V, negative_slope, &drop, &ee);
}

// graphop_gat_attention_backward (drop == nullptr), its dropout form or, with the edge term ee (which needs drop),
// graphop_gat_edge_attention_backward, as `fn`: -> {del, der, dV}, with ee {del, der, dee, dV}
std::vector<at::Tensor> gat_attention_backward_impl(const char* fn, const at::Tensor& row, const at::Tensor& indptr_r,
                                                    const at::Tensor& eid_r, const at::Tensor& indices_r,
                                                    const at::Tensor& col, const at::Tensor& indptr_c,
                                                    const at::Tensor& eid_c, const at::Tensor& indices_c,
                                                    const at::Tensor& el, const at::Tensor& er, const at::Tensor& V,
                                                    const at::Tensor& o, const at::Tensor& stats,
                                                    const at::Tensor& dO_, double negative_slope, const DropSpec* drop,
                                                    const at::Tensor* ee = nullptr, bool need_dee = true) {
  CHECK_CSR(row, indptr_r, eid_r, indices_r);
  CHECK_CSR(col, indptr_c, eid_c, indices_c);
  CHECK_INPUT(el); CHECK_INPUT(er); CHECK_INPUT(V); CHECK_INPUT(o); CHECK_INPUT(stats);
  CHECK_CUDA(dO_);
  const auto hd = gat_attn_shapes(el, er, V, fn);
  const int64_t h = hd.first, d = hd.second;
  const int64_t e = eid_r.size(0), n_l = el.size(0);
  if (ee) gat_edge_term(el, *ee, e, h, fn);
  CHECK_SAME_DTYPE(el, o); CHECK_SAME_DTYPE(el, stats); CHECK_SAME_DTYPE(el, dO_);
  const at::Tensor dO = saved_checked(fn, with_rows(V, n_l), n_l, h, o, stats, dO_);
  DeviceGuard dg(el);
  auto d_el = at::empty_like(el), d_er = at::empty_like(er), dV = at::empty_like(V);
  auto ws = at::empty({std::max<int64_t>(n_l * h * 4, 1)}, el.options());   // (el, m, 1 / l, D) per (node, head)
  const auto ppr = get_plan(row, indptr_r, eid_r, indices_r, er.size(0));
  const auto ppc = get_plan(col, indptr_c, eid_c, indices_c, n_l);
  const auto &pr = *ppr, &pc = *ppc;
  if (ee) {
    auto d_ee = need_dee ? at::empty_like(*ee) : at::empty({0}, ee->options());   // the only edge-sized tensor made
    check(graphop_gat_edge_attention_backward(
        dtype_code(el), ip(row), ip(indptr_r), ip(eid_r), ip(indices_r), ip(col), ip(indptr_c), ip(eid_c),
        ip(indices_c), vp(el), vp(er), vp(*ee), vp(V), vp(o), vp(stats), vp(dO), vp(d_el), vp(d_er),
        need_dee ? vp(d_ee) : nullptr, vp(dV), vp(ws), ws.numel() * ws.element_size(), row.size(0), col.size(0), e, n_l,
        er.size(0), h, d, negative_slope, drop->p, drop->seed, drop->offset, pr.plan, pc.plan, stream_of(el)));
    return {d_el, d_er, d_ee, dV};
  }
  if (drop)
    check(graphop_gat_attention_dropout_backward(
        dtype_code(el), ip(row), ip(indptr_r), ip(eid_r), ip(indices_r), ip(col), ip(indptr_c), ip(eid_c),
        ip(indices_c), vp(el), vp(er), vp(V), vp(o), vp(stats), vp(dO), vp(d_el), vp(d_er), vp(dV), vp(ws),
        ws.numel() * ws.element_size(), row.size(0), col.size(0), e, n_l, er.size(0), h, d, negative_slope, drop->p,
        drop->seed, drop->offset, pr.plan, pc.plan, stream_of(el)));
  else
    check(graphop_gat_attention_backward(dtype_code(el), ip(row), ip(indptr_r), ip(eid_r), ip(indices_r), ip(col),
                                         ip(indptr_c), ip(eid_c), ip(indices_c), vp(el), vp(er), vp(V), vp(o),
                                         vp(stats), vp(dO), vp(d_el), vp(d_er), vp(dV), vp(ws),
                                         ws.numel() * ws.element_size(), row.size(0), col.size(0), e, n_l, er.size(0),
                                         h, d, negative_slope, pr.plan, pc.plan, stream_of(el)));
  return {d_el, d_er, dV};
}

std::vector<at::Tensor> gat_attention_backward(const at::Tensor& row, const at::Tensor& indptr_r,
                                               const at::Tensor& eid_r, const at::Tensor& indices_r,
                                               const at::Tensor& col, const at::Tensor& indptr_c,
                                               const at::Tensor& eid_c, const at::Tensor& indices_c,
                                               const at::Tensor& el, const at::Tensor& er, const at::Tensor& V,
                                               const at::Tensor& o, const at::Tensor& stats, const at::Tensor& dO,
                                               double negative_slope) {
  return gat_attention_backward_impl("gat_attention_backward", row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c,
                                     indices_c, el, er, V, o, stats, dO, negative_slope, nullptr);
}

std::vector<at::Tensor> gat_attention_dropout_backward(const at::Tensor& row, const at::Tensor& indptr_r,
                                                       const at::Tensor& eid_r, const at::Tensor& indices_r,
                                                       const at::Tensor& col, const at::Tensor& indptr_c,
                                                       const at::Tensor& eid_c, const at::Tensor& indices_c,
                                                       const at::Tensor& el, const at::Tensor& er, const at::Tensor& V,
                                                       const at::Tensor& o, const at::Tensor& stats,
                                                       const at::Tensor& dO, double negative_slope, double p,
                                                       int64_t seed, int64_t offset) {
  const char* fn = "gat_attention_dropout_backward";
  const DropSpec drop = drop_spec(fn, p, seed, offset);
  return gat_attention_backward_impl(fn, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, V,
                                     o, stats, dO, negative_slope, &drop);
}

std::vector<at::Tensor> gat_edge_attention_backward(const at::Tensor& row, const at::Tensor& indptr_r,
                                                    const at::Tensor& eid_r, const at::Tensor& indices_r,
                                                    const at::Tensor& col, const at::Tensor& indptr_c,
                                                    const at::Tensor& eid_c, const at::Tensor& indices_c,
                                                    const at::Tensor& el, const at::Tensor& er, const at::Tensor& ee,
                                                    const at::Tensor& V, const at::Tensor& o, const at::Tensor& stats,
                                                    const at::Tensor& dO, double negative_slope, double p,
                                                    int64_t seed, int64_t offset, bool need_dee) {
  const char* fn = "gat_edge_attention_backward";
  const DropSpec drop = drop_spec(fn, p, seed, offset);
  return gat_attention_backward_impl(fn, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, V,
                                     o, stats, dO, negative_slope, &drop, &ee, need_dee);
}

// ---- the weights of the fused GAT / GATv2 layers from their row statistics (include/graphop_hip.h:
// graphop_gat_attention_weights, graphop_gatv2_attention_weights) ---------------------------------------------------
// stats (n_src, h, 2) in the dtype of the row-side operand first (el or xl)
#define CHECK_GAT_WEIGHTS_STATS(fn, first, stats, h)                                                              \
  CHECK_SAME_DTYPE(first, stats);                                                                                 \
  TORCH_CHECK((stats).dim() == 3 && (stats).size(0) == (first).size(0) && (stats).size(1) == (h) &&              \
              (stats).size(2) == 2, fn, ": stats must be (n_src, h, 2) = (", (first).size(0), ", ", (h),         \
              ", 2), got ", (stats).sizes())

at::Tensor gat_attention_weights(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                                 const at::Tensor& indices, const at::Tensor& el, const at::Tensor& er,
                                 const at::Tensor& stats, const c10::optional<at::Tensor>& ee, double negative_slope) {
  const char* fn = "gat_attention_weights";
  CHECK_CSR(row, indptr, eid, indices);
  CHECK_INPUT(el); CHECK_INPUT(er); CHECK_INPUT(stats);
  const int64_t h = gat_heads(el, er, fn);
  const int64_t e = eid.size(0);
  CHECK_GAT_WEIGHTS_STATS(fn, el, stats, h);
  if (ee) gat_edge_term(el, *ee, e, h, fn);
  DeviceGuard dg(el);
  const auto pp = get_plan(row, indptr, eid, indices, er.size(0));
  const auto& pl = *pp;
  // a[e] is written once per row-major slot: only a chunk list that leaves slots out needs the zeros
  const std::vector<int64_t> shape = el.dim() == 1 ? std::vector<int64_t>{e} : std::vector<int64_t>{e, h};
  auto a = pl.info.full_coverage ? at::empty(shape, el.options()) : at::zeros(shape, el.options());
  check(graphop_gat_attention_weights(dtype_code(el), ip(row), ip(indptr), ip(eid), ip(indices), vp(el), vp(er),
                                      ee ? vp(*ee) : nullptr, vp(stats), vp(a), row.size(0), e, el.size(0), er.size(0),
                                      h, negative_slope, pl.plan, stream_of(el)));
  return a;
}

at::Tensor gatv2_attention_weights(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                                   const at::Tensor& indices, const at::Tensor& xl, const at::Tensor& xr,
                                   const at::Tensor& att, const at::Tensor& stats,
                                   const c10::optional<at::Tensor>& xe, double negative_slope) {
  const char* fn = "gatv2_attention_weights";
  CHECK_CSR(row, indptr, eid, indices);
  CHECK_INPUT(xl); CHECK_INPUT(xr); CHECK_INPUT(att); CHECK_INPUT(stats);
  const auto hd = gatv2_shapes(xl, xr, att, fn);
  const int64_t h = hd.first, d = hd.second;
  const int64_t e = eid.size(0);
  CHECK_GAT_WEIGHTS_STATS(fn, xl, stats, h);
  if (xe) gatv2_edge_rows(xl, *xe, e, h, d, fn);
  DeviceGuard dg(xl);
  const auto pp = get_plan(row, indptr, eid, indices, xr.size(0));
  const auto& pl = *pp;
  const std::vector<int64_t> shape = xl.dim() == 2 ? std::vector<int64_t>{e} : std::vector<int64_t>{e, h};
  auto a = pl.info.full_coverage ? at::empty(shape, xl.options()) : at::zeros(shape, xl.options());
  check(graphop_gatv2_attention_weights(dtype_code(xl), ip(row), ip(indptr), ip(eid), ip(indices), vp(xl), vp(xr),
                                        xe ? vp(*xe) : nullptr, vp(att), vp(stats), vp(a), row.size(0), e, xl.size(0),
                                        xr.size(0), h, d, negative_slope, pl.plan, stream_of(xl)));
  return a;
}

// m[e, k] = keep(i, j, k) / (1 - p) of the dropout forms as an edge tensor, over the row-major CSR
at::Tensor edge_dropout_mask(const at::Tensor& row, const at::Tensor& indptr, const at::Tensor& eid,
                             const at::Tensor& indices, int64_t h, double p, int64_t seed, int64_t offset,
                             at::ScalarType dtype) {
  const DropSpec drop = drop_spec("edge_dropout_mask", p, seed, offset);
  CHECK_CSR(row, indptr, eid, indices);
  TORCH_CHECK(h >= 1 && (dtype == at::kFloat || dtype == at::kDouble),
              "edge_dropout_mask: h must be >= 1 and dtype float32 or float64, got h=", h, " dtype=", dtype);
  DeviceGuard dg(row);
  const int64_t e = eid.size(0);
  auto y = at::empty(h == 1 ? std::vector<int64_t>{e} : std::vector<int64_t>{e, h}, row.options().dtype(dtype));
  const auto pp = get_plan(row, indptr, eid, indices, 0);
  const auto& pl = *pp;
  const int64_t cap = (int64_t(1) << 32) - 1;   // the ids themselves are the only bound on the two node counts
  const int64_t n_l = e ? std::min<int64_t>(std::max<int64_t>(pl.info.max_row + 1, 0), cap) : 0;
  const int64_t n_r = e ? std::min<int64_t>(std::max<int64_t>(pl.info.max_index + 1, 0), cap) : 0;
  check(graphop_edge_dropout_mask(dtype_code(y), ip(row), ip(indptr), ip(eid), ip(indices), vp(y), row.size(0), e, n_l,
                                  n_r, h, drop.p, drop.seed, drop.offset, pl.plan, stream_of(row)));
  return y;
}

void clear_plan_cache() {
  std::vector<PlanRef> dead;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto& kv : g_graphs)
      for (auto& p : kv.second.plans) dead.push_back(std::move(p));
    g_graphs.clear();
    g_lru.clear();
  }
}

// drop the plans of the orientation whose chunk list is `row` (graphs.release)
void release_plans(const at::Tensor& row) {
  std::vector<PlanRef> dead;
  const void* r = row.numel() ? row.data_ptr() : nullptr;
  std::lock_guard<std::mutex> lk(g_mu);
  for (auto it = g_graphs.begin(); it != g_graphs.end();) {
    if (it->first.row == r) {
      for (auto& p : it->second.plans) dead.push_back(std::move(p));
      g_lru.erase(it->second.lru);
      it = g_graphs.erase(it);
    } else {
      ++it;
    }
  }
}

int64_t plan_cache_size() {
  std::lock_guard<std::mutex> lk(g_mu);
  return (int64_t)g_graphs.size();
}

// ---- registration 1: the reference's pybind11 module (graphop.cpp:216-225) ------------------------------
PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("maskedmm_csr_forward", &maskedmm_csr_forward, "Masked Matrix Multiplication forward(CSR Format)");
  m.def("maskedmm_csr_backward", &maskedmm_csr_backward, "Masked Matrix Multiplication backward(CSR Format)");
  m.def("node_mul_edge_forward", &node_mul_edge_forward, "Node Multiply Edge forward");
  m.def("node_mul_edge_backward", &node_mul_edge_backward, "Node Multiply Edge backward");
  m.def("sparse_softmax_forward", &sparse_softmax_forward, "Sparse softmax forward");
  m.def("sparse_softmax_backward", &sparse_softmax_backward, "Sparse softmax backward");
  m.def("vector_spmm_forward", &vector_spmm_forward, "Vectorized SPMM forward");
  m.def("vector_spmm_backward", &vector_spmm_backward, "Vectorized SPMM backward");
  m.def("attention_forward", &attention_forward, "Fused SDDMM -> softmax -> SpMM forward (extra op)");
  m.def("attention_backward", &attention_backward, "Fused attention backward (extra op)");
  // (the dropout form of the fused step is bound here and by ctypes; it is not in the torch.ops.graphop table below)
  m.def("attention_dropout_forward", &attention_dropout_forward,
        "Fused attention forward with attention dropout (extra op)", py::arg("row"), py::arg("indptr"), py::arg("eid"),
        py::arg("indices"), py::arg("Q"), py::arg("K"), py::arg("V"), py::arg("p") = 0.0, py::arg("seed") = 0,
        py::arg("offset") = 0, py::arg("head0") = 0);
  m.def("attention_dropout_backward", &attention_dropout_backward,
        "Fused attention backward with attention dropout (extra op)", py::arg("row"), py::arg("indptr_r"),
        py::arg("eid_r"), py::arg("indices_r"), py::arg("col"), py::arg("indptr_c"), py::arg("eid_c"),
        py::arg("indices_c"), py::arg("Q"), py::arg("K"), py::arg("V"), py::arg("o"), py::arg("stats"), py::arg("dO"),
        py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("offset") = 0, py::arg("head0") = 0);
  // (likewise its form with a per-edge score bias)
  m.def("attention_bias_forward", &attention_bias_forward,
        "Fused attention forward with a per-edge score bias (extra op)", py::arg("row"), py::arg("indptr"), py::arg("eid"),
        py::arg("indices"), py::arg("Q"), py::arg("K"), py::arg("V"), py::arg("b"), py::arg("p") = 0.0,
        py::arg("seed") = 0, py::arg("offset") = 0, py::arg("head0") = 0);
  m.def("attention_bias_backward", &attention_bias_backward,
        "Fused attention backward with a per-edge score bias (extra op)", py::arg("row"), py::arg("indptr_r"),
        py::arg("eid_r"), py::arg("indices_r"), py::arg("col"), py::arg("indptr_c"), py::arg("eid_c"),
        py::arg("indices_c"), py::arg("Q"), py::arg("K"), py::arg("V"), py::arg("b"), py::arg("o"), py::arg("stats"),
        py::arg("dO"), py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("offset") = 0, py::arg("head0") = 0,
        py::arg("need_db") = true);
  // (likewise its form with edge features: K_j + xe[e], V_j + xe[e])
  m.def("attention_edge_forward", &attention_edge_forward,
        "Fused attention forward with edge features in key and value (extra op)", py::arg("row"), py::arg("indptr"),
        py::arg("eid"), py::arg("indices"), py::arg("Q"), py::arg("K"), py::arg("V"), py::arg("xe"), py::arg("p") = 0.0,
        py::arg("seed") = 0, py::arg("offset") = 0, py::arg("head0") = 0);
  m.def("attention_edge_backward", &attention_edge_backward,
        "Fused attention backward with edge features in key and value (extra op)", py::arg("row"), py::arg("indptr_r"),
        py::arg("eid_r"), py::arg("indices_r"), py::arg("col"), py::arg("indptr_c"), py::arg("eid_c"),
        py::arg("indices_c"), py::arg("Q"), py::arg("K"), py::arg("V"), py::arg("xe"), py::arg("o"), py::arg("stats"),
        py::arg("dO"), py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("offset") = 0, py::arg("head0") = 0,
        py::arg("need_dxe") = true);
  // (likewise its form with edge-type embeddings: K_j + R[etype[e]], V_j + R[etype[e]])
  m.def("attention_etype_forward", &attention_etype_forward,
        "Fused attention forward with edge-type embeddings in key and value (extra op)", py::arg("row"),
        py::arg("indptr"), py::arg("eid"), py::arg("indices"), py::arg("Q"), py::arg("K"), py::arg("V"), py::arg("R"),
        py::arg("etype"), py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("offset") = 0, py::arg("head0") = 0);
  m.def("attention_etype_backward", &attention_etype_backward,
        "Fused attention backward with edge-type embeddings in key and value (extra op)", py::arg("row"),
        py::arg("indptr_r"), py::arg("eid_r"), py::arg("indices_r"), py::arg("col"), py::arg("indptr_c"),
        py::arg("eid_c"), py::arg("indices_c"), py::arg("Q"), py::arg("K"), py::arg("V"), py::arg("R"), py::arg("etype"),
        py::arg("o"), py::arg("stats"), py::arg("dO"), py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("offset") = 0,
        py::arg("head0") = 0, py::arg("need_dR") = true);
  // (and its form with an edge-type score bias: <Q_i, K_j> + B[etype[e], k])
  m.def("attention_tbias_forward", &attention_tbias_forward,
        "Fused attention forward with an edge-type score bias (extra op)", py::arg("row"), py::arg("indptr"),
        py::arg("eid"), py::arg("indices"), py::arg("Q"), py::arg("K"), py::arg("V"), py::arg("B"),
        py::arg("etype"), py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("offset") = 0, py::arg("head0") = 0);
  m.def("attention_tbias_backward", &attention_tbias_backward,
        "Fused attention backward with an edge-type score bias (extra op)", py::arg("row"),
        py::arg("indptr_r"), py::arg("eid_r"), py::arg("indices_r"), py::arg("col"), py::arg("indptr_c"),
        py::arg("eid_c"), py::arg("indices_c"), py::arg("Q"), py::arg("K"), py::arg("V"), py::arg("B"), py::arg("etype"),
        py::arg("o"), py::arg("stats"), py::arg("dO"), py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("offset") = 0,
        py::arg("head0") = 0, py::arg("need_dB") = true);
  // (and the weights of all of these from their row statistics)
  m.def("attention_weights", &attention_weights,
        "Attention weights of the fused attention ops from their row statistics (extra op)", py::arg("row"),
        py::arg("indptr"), py::arg("eid"), py::arg("indices"), py::arg("Q"), py::arg("K"), py::arg("stats"),
        py::arg("b") = py::none(), py::arg("xe") = py::none());
  m.def("gat_scores_forward", &gat_scores_forward, "GAT additive attention scores forward (extra op)", py::arg("row"),
        py::arg("indptr"), py::arg("eid"), py::arg("indices"), py::arg("el"), py::arg("er"), py::arg("negative_slope") = 0.2);
  m.def("gat_scores_backward", &gat_scores_backward, "GAT additive attention scores backward (extra op)", py::arg("row"),
        py::arg("indptr_r"), py::arg("eid_r"), py::arg("indices_r"), py::arg("col"), py::arg("indptr_c"), py::arg("eid_c"),
        py::arg("indices_c"), py::arg("el"), py::arg("er"), py::arg("dy"), py::arg("negative_slope") = 0.2);
  m.def("gat_attention_forward", &gat_attention_forward, "Fused GAT attention forward (extra op)", py::arg("row"),
        py::arg("indptr"), py::arg("eid"), py::arg("indices"), py::arg("el"), py::arg("er"), py::arg("V"),
        py::arg("negative_slope") = 0.2);
  m.def("gat_attention_backward", &gat_attention_backward, "Fused GAT attention backward (extra op)", py::arg("row"),
        py::arg("indptr_r"), py::arg("eid_r"), py::arg("indices_r"), py::arg("col"), py::arg("indptr_c"), py::arg("eid_c"),
        py::arg("indices_c"), py::arg("el"), py::arg("er"), py::arg("V"), py::arg("o"), py::arg("stats"), py::arg("dO"),
        py::arg("negative_slope") = 0.2);
  m.def("gat_attention_dropout_forward", &gat_attention_dropout_forward,
        "Fused GAT attention forward with attention dropout (extra op)", py::arg("row"), py::arg("indptr"),
        py::arg("eid"), py::arg("indices"), py::arg("el"), py::arg("er"), py::arg("V"), py::arg("negative_slope") = 0.2,
        py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("offset") = 0);
  m.def("gat_attention_dropout_backward", &gat_attention_dropout_backward,
        "Fused GAT attention backward with attention dropout (extra op)", py::arg("row"), py::arg("indptr_r"),
        py::arg("eid_r"), py::arg("indices_r"), py::arg("col"), py::arg("indptr_c"), py::arg("eid_c"),
        py::arg("indices_c"), py::arg("el"), py::arg("er"), py::arg("V"), py::arg("o"), py::arg("stats"), py::arg("dO"),
        py::arg("negative_slope") = 0.2, py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("offset") = 0);
  m.def("edge_dropout_mask", &edge_dropout_mask, "The dropout multipliers of the fused GAT layer as an edge tensor",
        py::arg("row"), py::arg("indptr"), py::arg("eid"), py::arg("indices"), py::arg("h"), py::arg("p") = 0.0,
        py::arg("seed") = 0, py::arg("offset") = 0, py::arg("dtype") = at::kFloat);
  m.def("gatv2_scores_forward", &gatv2_scores_forward, "GATv2 attention scores forward (extra op)", py::arg("row"),
        py::arg("indptr"), py::arg("eid"), py::arg("indices"), py::arg("xl"), py::arg("xr"), py::arg("att"),
        py::arg("negative_slope") = 0.2);
  m.def("gatv2_scores_backward", &gatv2_scores_backward, "GATv2 attention scores backward (extra op)", py::arg("row"),
        py::arg("indptr_r"), py::arg("eid_r"), py::arg("indices_r"), py::arg("col"), py::arg("indptr_c"), py::arg("eid_c"),
        py::arg("indices_c"), py::arg("xl"), py::arg("xr"), py::arg("att"), py::arg("dy"), py::arg("negative_slope") = 0.2);
  m.def("gatv2_attention_forward", &gatv2_attention_forward, "Fused GATv2 attention forward (extra op)", py::arg("row"),
        py::arg("indptr"), py::arg("eid"), py::arg("indices"), py::arg("xl"), py::arg("xr"), py::arg("att"),
        py::arg("negative_slope") = 0.2);
  m.def("gatv2_attention_backward", &gatv2_attention_backward, "Fused GATv2 attention backward (extra op)",
        py::arg("row"), py::arg("indptr_r"), py::arg("eid_r"), py::arg("indices_r"), py::arg("col"), py::arg("indptr_c"),
        py::arg("eid_c"), py::arg("indices_c"), py::arg("xl"), py::arg("xr"), py::arg("att"), py::arg("o"),
        py::arg("stats"), py::arg("dO"), py::arg("negative_slope") = 0.2);
  m.def("gatv2_attention_dropout_forward", &gatv2_attention_dropout_forward,
        "Fused GATv2 attention forward with attention dropout (extra op)", py::arg("row"), py::arg("indptr"),
        py::arg("eid"), py::arg("indices"), py::arg("xl"), py::arg("xr"), py::arg("att"),
        py::arg("negative_slope") = 0.2, py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("offset") = 0,
        py::arg("xe") = py::none());
  m.def("gatv2_attention_dropout_backward", &gatv2_attention_dropout_backward,
        "Fused GATv2 attention backward with attention dropout (extra op)", py::arg("row"), py::arg("indptr_r"),
        py::arg("eid_r"), py::arg("indices_r"), py::arg("col"), py::arg("indptr_c"), py::arg("eid_c"),
        py::arg("indices_c"), py::arg("xl"), py::arg("xr"), py::arg("att"), py::arg("o"), py::arg("stats"),
        py::arg("dO"), py::arg("negative_slope") = 0.2, py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("offset") = 0,
        py::arg("xe") = py::none(), py::arg("need_dxe") = true);
  m.def("gat_edge_attention_forward", &gat_edge_attention_forward,
        "Fused GAT attention with an edge term, forward (extra op)", py::arg("row"), py::arg("indptr"), py::arg("eid"),
        py::arg("indices"), py::arg("el"), py::arg("er"), py::arg("ee"), py::arg("V"), py::arg("negative_slope") = 0.2,
        py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("offset") = 0);
  m.def("gat_edge_attention_backward", &gat_edge_attention_backward,
        "Fused GAT attention with an edge term, backward (extra op)", py::arg("row"), py::arg("indptr_r"),
        py::arg("eid_r"), py::arg("indices_r"), py::arg("col"), py::arg("indptr_c"), py::arg("eid_c"),
        py::arg("indices_c"), py::arg("el"), py::arg("er"), py::arg("ee"), py::arg("V"), py::arg("o"), py::arg("stats"),
        py::arg("dO"), py::arg("negative_slope") = 0.2, py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("offset") = 0,
        py::arg("need_dee") = true);
  // (and the weights of the six fused GAT / GATv2 layers from their row statistics)
  m.def("gat_attention_weights", &gat_attention_weights,
        "Attention weights of the fused GAT layers from their row statistics (extra op)", py::arg("row"),
        py::arg("indptr"), py::arg("eid"), py::arg("indices"), py::arg("el"), py::arg("er"), py::arg("stats"),
        py::arg("ee") = py::none(), py::arg("negative_slope") = 0.2);
  m.def("gatv2_attention_weights", &gatv2_attention_weights,
        "Attention weights of the fused GATv2 layers from their row statistics (extra op)", py::arg("row"),
        py::arg("indptr"), py::arg("eid"), py::arg("indices"), py::arg("xl"), py::arg("xr"), py::arg("att"),
        py::arg("stats"), py::arg("xe") = py::none(), py::arg("negative_slope") = 0.2);
  m.def("clear_plan_cache", &clear_plan_cache, "Destroy every cached per-graph plan");
  m.def("release_plans", &release_plans, "Drop the cached plans of the orientation whose chunk list is `row`");
  m.def("plan_cache_size", &plan_cache_size, "Graph orientations in the plan cache");
}

// ---- registration 2: torch.ops.graphop.* (schemas + CUDA(HIP) implementations) ------------------------------
// One row per op: its name, which is also its function's, and its schema (graphop.py's _SCHEMAS holds the same text
// for the ctypes binding).  The rows expand into the definitions and into both dispatch keys below.
#define GRAPHOP_OPS(X) \
  X(maskedmm_csr_forward, "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor A, Tensor B) -> Tensor") \
  X(maskedmm_csr_backward, "(Tensor row, Tensor indptr_r, Tensor eid_r, Tensor indices_r, Tensor col, Tensor indptr_c, Tensor eid_c, Tensor indices_c, Tensor A, Tensor B, Tensor dy) -> Tensor[]") \
  X(node_mul_edge_forward, "(Tensor row, Tensor indptr, Tensor eid, Tensor A, Tensor B) -> Tensor") \
  X(node_mul_edge_backward, "(Tensor row, Tensor indptr, Tensor eid, Tensor A, Tensor B, Tensor dy) -> Tensor[]") \
  X(sparse_softmax_forward, "(Tensor row, Tensor indptr, Tensor eid, Tensor x) -> Tensor") \
  X(sparse_softmax_backward, "(Tensor row, Tensor indptr, Tensor eid, Tensor y, Tensor dy) -> Tensor") \
  X(vector_spmm_forward, "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor edata, Tensor x) -> Tensor") \
  X(vector_spmm_backward, "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor col, Tensor indptr_t, Tensor eid_t, Tensor indices_t, Tensor edata, Tensor dy, Tensor x) -> Tensor[]") \
  X(attention_forward, "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor Q, Tensor K, Tensor V) -> Tensor[]") \
  X(attention_backward, "(Tensor row, Tensor indptr_r, Tensor eid_r, Tensor indices_r, Tensor col, Tensor indptr_c, Tensor eid_c, Tensor indices_c, Tensor Q, Tensor K, Tensor V, Tensor o, Tensor stats, Tensor dO) -> Tensor[]") \
  X(gat_scores_forward, "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor el, Tensor er, float negative_slope=0.2) -> Tensor") \
  X(gat_scores_backward, "(Tensor row, Tensor indptr_r, Tensor eid_r, Tensor indices_r, Tensor col, Tensor indptr_c, Tensor eid_c, Tensor indices_c, Tensor el, Tensor er, Tensor dy, float negative_slope=0.2) -> Tensor[]") \
  X(gat_attention_forward, "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor el, Tensor er, Tensor V, float negative_slope=0.2) -> Tensor[]") \
  X(gat_attention_backward, "(Tensor row, Tensor indptr_r, Tensor eid_r, Tensor indices_r, Tensor col, Tensor indptr_c, Tensor eid_c, Tensor indices_c, Tensor el, Tensor er, Tensor V, Tensor o, Tensor stats, Tensor dO, float negative_slope=0.2) -> Tensor[]") \
  X(gat_attention_dropout_forward, "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor el, Tensor er, Tensor V, float negative_slope=0.2, float p=0.0, int seed=0, int offset=0) -> Tensor[]") \
  X(gat_attention_dropout_backward, "(Tensor row, Tensor indptr_r, Tensor eid_r, Tensor indices_r, Tensor col, Tensor indptr_c, Tensor eid_c, Tensor indices_c, Tensor el, Tensor er, Tensor V, Tensor o, Tensor stats, Tensor dO, float negative_slope=0.2, float p=0.0, int seed=0, int offset=0) -> Tensor[]") \
  X(edge_dropout_mask, "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, int h, float p=0.0, int seed=0, int offset=0, ScalarType dtype=float) -> Tensor") \
  X(gatv2_scores_forward, "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor xl, Tensor xr, Tensor att, float negative_slope=0.2) -> Tensor") \
  X(gatv2_scores_backward, "(Tensor row, Tensor indptr_r, Tensor eid_r, Tensor indices_r, Tensor col, Tensor indptr_c, Tensor eid_c, Tensor indices_c, Tensor xl, Tensor xr, Tensor att, Tensor dy, float negative_slope=0.2) -> Tensor[]") \
  X(gatv2_attention_forward, "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor xl, Tensor xr, Tensor att, float negative_slope=0.2) -> Tensor[]") \
  X(gatv2_attention_backward, "(Tensor row, Tensor indptr_r, Tensor eid_r, Tensor indices_r, Tensor col, Tensor indptr_c, Tensor eid_c, Tensor indices_c, Tensor xl, Tensor xr, Tensor att, Tensor o, Tensor stats, Tensor dO, float negative_slope=0.2) -> Tensor[]") \
  X(gatv2_attention_dropout_forward, "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor xl, Tensor xr, Tensor att, float negative_slope=0.2, float p=0.0, int seed=0, int offset=0, Tensor? xe=None) -> Tensor[]") \
  X(gatv2_attention_dropout_backward, "(Tensor row, Tensor indptr_r, Tensor eid_r, Tensor indices_r, Tensor col, Tensor indptr_c, Tensor eid_c, Tensor indices_c, Tensor xl, Tensor xr, Tensor att, Tensor o, Tensor stats, Tensor dO, float negative_slope=0.2, float p=0.0, int seed=0, int offset=0, Tensor? xe=None, bool need_dxe=True) -> Tensor[]") \
  X(gat_edge_attention_forward, "(Tensor row, Tensor indptr, Tensor eid, Tensor indices, Tensor el, Tensor er, Tensor ee, Tensor V, float negative_slope=0.2, float p=0.0, int seed=0, int offset=0) -> Tensor[]") \
  X(gat_edge_attention_backward, "(Tensor row, Tensor indptr_r, Tensor eid_r, Tensor indices_r, Tensor col, Tensor indptr_c, Tensor eid_c, Tensor indices_c, Tensor el, Tensor er, Tensor ee, Tensor V, Tensor o, Tensor stats, Tensor dO, float negative_slope=0.2, float p=0.0, int seed=0, int offset=0, bool need_dee=True) -> Tensor[]")
#define GRAPHOP_DEF(name, schema) m.def(#name schema);
#define GRAPHOP_IMPL(name, schema) m.impl(#name, &name);

TORCH_LIBRARY(graphop, m) { GRAPHOP_OPS(GRAPHOP_DEF) }

TORCH_LIBRARY_IMPL(graphop, CUDA, m) { GRAPHOP_OPS(GRAPHOP_IMPL) }

// there is no CPU implementation: the reference's CHECK_CUDA message
TORCH_LIBRARY_IMPL(graphop, CPU, m) { GRAPHOP_OPS(GRAPHOP_IMPL) }
