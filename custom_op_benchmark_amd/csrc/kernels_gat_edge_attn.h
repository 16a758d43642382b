// Fused GAT attention with an edge term (extra op, not in the reference; gat_edge_attention.hip has the entry points):
//   z_e = (el[i] + er[j]) + ee[e],  s = LeakyReLU(z),  a = row-softmax(s),  o[i] = sum_j a_ij m_ij V[j]   (per head k)
// for edge e = (i, j); ee is indexed by edge id, so a slot reads ee[eid[slot]].  m_ij is the dropout multiplier of
// kernels_dropout.h (1 without dropout).  The backward is that of kernels_gat_attn.h plus one output:
//   dz_e = a (da - D) * (z > 0 ? 1 : slope),  del[i] = sum_j dz,  der[j] = sum_i dz,  dV[j] = sum_i a m dO_i,  dee[e] = dz_e
// dee is the only edge-sized tensor written: one plain store per slot and head from the row-major pass, where every
// slot is visited once.  The passes are the text of kernels_gat_attn_passes.inc compiled a second time, with the edge
// term: every gather pass additionally reads the slot's edge id and the h values of ee.  The pack kernels and the
// generic stats init / finish of kernels_gat_attn.h are launched unchanged: P = (el, m, 1/l, D) still holds.
// A NULL eid means eid[slot] == slot (a plan with eid_identity, as graph_from_coo always yields in row-major order):
// a kernel-uniform branch, not a second set of instantiations.
#pragma once
#include "kernels_gat_attn.h"

namespace graphop {

#define GA_EDGE 1
#define GA_KERNEL(pass, kind) k_gat_edge_attn_##pass##_##kind
#define GA_FN(name) gat_edge_attn_##name
#include "kernels_gat_attn_passes.inc"
#undef GA_EDGE
#undef GA_KERNEL
#undef GA_FN

}  // namespace graphop
