// TILE driver of the SDDMM-type passes (fp32, one head, 256-B rows, identity eid, table < 4 GiB):
// a WORKGROUP takes a (column window, row tile) task of R vrows and gathers every neighbour row the tile touches in that
// window ONCE -- the window-owner strips (kernels_wown.h) gather it once per slot, and a wave's 32 vrows share few
// neighbours; R = 192 vrows of the Reddit shape share 24 % of their slots' neighbours (R = 384: 37 %).  A result is per
// edge, so the task's slots may be processed in any order: the plan stores them grouped by neighbour id (tile_layout.h: column
// records of <= 4 slots, 16 records per batch, batches of equal slot counts first).
// Per task: the R A rows -> LDS; every 16-lane group takes batches of 16 records, requests the 16 neighbour rows, and
// for slot k = 0 .. 3 of the records runs the strips' 16-slot transpose-reduce (the same summation tree: a result is
// bitwise what the strips store) with the A row of each record's k-th slot; results go to the task's result buffer in
// LDS, no global store stands between row requests.  After a barrier the workgroup copies every vrow's run of results
// to y + (first edge id of the run).  Every result is written exactly once with a plain store: a stolen task needs no
// atomics, y no zero fill.  Waves meet only in __syncthreads: no spin waits, no hand-overs.
#pragma once
#include "kernels_wown.h"

namespace graphop {

struct TileView {
  const int* part_ptr;   // [W * tiles + 1]
  const int4* parts;     // (first batch, records, first row in tile, rows)
  const unsigned short* rec;   // [16 * batches] ((neighbour id - first id of the window) << 2) | (slots - 1)
  const int* bstart;     // [batches] first slot word of the batch
  const int* slotw;      // (row in tile << 16) | result offset
  const int2* rowtab;    // [W * V] (first edge id, result offset | slots << 16)
  const int4* tdesc;     // [W * tiles] (first batch, batches, first slot word, slot words) of every task
  const int* vr_row;     // [V]
  int* sync;             // the eight per-XCD queue heads (WownQueue), zeroed before the launch
  int V, W, R, tiles;
  int win_cols;          // ids per window (<= 16384)
  int touch;             // 1: one wave touches the NEXT task's record and slot-word lines while this task runs
};

constexpr int kTileLdsBytes = 158 * 1024;   // A rows + result buffer of one workgroup, or of the two that share a CU

// inclusive sum over the lanes 0 .. l of a 16-lane DPP row (row_shr: lanes shifted in from outside the row read 0)
__device__ __forceinline__ int row16_incl_scan(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);
  return v;
}
__device__ __forceinline__ int row16_max(int v) {
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true));
  return v;
}

// 16 bytes per lane from memory straight into LDS (gfx950: global_load_lds_dwordx4; no destination register).  src is per
// lane; the destination is wave_base + lane x 16 B -- wave_base must be the same in every lane of the wave, and lanes that
// are switched off neither load nor write.  The load counts on vmcnt: wait for it before the barrier in front of the readers.
__device__ __forceinline__ void ld16_to_lds(const float* src, float4* wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)wave_base, 16, 0, 0);
}
__device__ __forceinline__ void wait_vmem() { __builtin_amdgcn_s_waitcnt(0x0F70); }   // gfx9 encoding: vmcnt(0), the other counters free

constexpr int kTileDescParts = 4;  // parts of a task whose records are handed over through LDS (a task rarely has two)

// NT threads per workgroup: 1024 (one workgroup per CU) or 512 (two per CU where their LDS packs); 16 waves per CU either way.
// Nothing a task needs first comes cold: its id is dequeued one task ahead (wave 0), its part records are fetched and the
// lines of its record, slot-word and row-table streams are touched into L2 by the LAST wave while the task in front of
// it runs; the lane groups take batches from an LDS counter, so that wave simply takes fewer.
//
// The two phases around a task's batch loop issue their memory requests together, not one row at a time.  STAGING: a lane
// group owns the RPG = R / G vrows g, g + G, ...; its lanes 0 .. RPG - 1 load one vrow's row-table entry and row id each
// (one round trip), the group broadcasts them and requests all its A rows back to back (a second round trip, one wait),
// straight into LDS.  WRITE-OUT: a group copies the vrows first + g, first + g + G, ... of a part, at most RPG of them; it
// requests all their row-table entries together when it leaves the batch loop (they arrive while it stands at the
// barrier) and then stores run after run with no load in between: loads and stores share vmcnt on gfx950, so a load per
// vrow made every vrow wait for the store acknowledgements of the vrow before it.
template <int L = 16, int NV = 1, int NT = 1024, int RPG = 4>
__global__ __launch_bounds__(NT, 4) void k_sddmm_tile_f32(TileView tv, const float* __restrict__ A,
                                                          const float* __restrict__ B, float* __restrict__ y) {
  static_assert(L == 16 && NV == 1, "256-B rows: one float4 per lane of a 16-lane group");
  static_assert(RPG >= 1 && RPG <= L, "one lane of a group per vrow entry");
  extern __shared__ float4 lds[];   // [R][L] A rows, then the result buffer
  __shared__ int task_sh[2][2];     // (window, tile) of the current and of the next task, by parity
  __shared__ int desc_sh[2][2 + 4 * kTileDescParts];   // first part, end part, the first parts' records, by parity
  __shared__ int ctr_sh;            // next batch of the part at hand
  constexpr int G = NT / L;
  constexpr int R = RPG * G;        // (= tv.R: launch_tile picks the instance)
  const int l = threadIdx.x % L, g = threadIdx.x / L;
  float* res = reinterpret_cast<float*>(lds + R * L);
  const char* lds_l = reinterpret_cast<const char*>(lds) + l * 16;
  SweepView qv{};
  qv.sync = tv.sync;
  qv.W = tv.W;
  WownQueue queue(qv, tv.tiles);
  // a wave fetches the part records of task (w, t) into desc_sh[slot] (lanes 0 .. 15 one int each)
  auto fetch_desc = [&](int slot, int w, int t) {
    const int lane = threadIdx.x & (kWave - 1);
    const i64 task = (i64)w * tv.tiles + t;
    const int p0 = tv.part_ptr[task], p1 = tv.part_ptr[task + 1];
    if (lane < 4 * kTileDescParts && p0 * 4 + lane < p1 * 4)
      desc_sh[slot][2 + lane] = reinterpret_cast<const int*>(tv.parts)[(i64)p0 * 4 + lane];
    if (lane == 0) { desc_sh[slot][0] = p0; desc_sh[slot][1] = p1; }
  };
  int raw = -1;
  if (threadIdx.x < kWave) {
    int w = -1, t = 0;
    const bool more = queue.pull(w, t);
    raw = more ? queue.issue() : -1;
    if (threadIdx.x == 0) { task_sh[0][0] = more ? w : -1; task_sh[0][1] = t; }
    if (more) fetch_desc(0, w, t);
  }
  auto next_batch = [&]() {   // group-uniform
    int v = 0;
    if (l == 0) v = atomicAdd(&ctr_sh, 1);
    return group_bcast<L, 0>(v);
  };
  int par = 0;
  for (;;) {
    __syncthreads();   // the task id is visible; the previous task's results have left the buffer, its A rows are free
    const int w = task_sh[par][0], t = task_sh[par][1];
    if (w < 0) break;
    if (threadIdx.x < kWave) {   // (the other parity's pair was last read before the previous task's second barrier)
      int wn = -1, tn = 0;
      const bool more = queue.resolve(raw, wn, tn);
      raw = more ? queue.issue() : -1;
      if (threadIdx.x == 0) { task_sh[par ^ 1][0] = more ? wn : -1; task_sh[par ^ 1][1] = tn; }
    }
    if (threadIdx.x == kWave) ctr_sh = 0;
    const int v0 = t * R;
    const int nr = (tv.V - v0) < R ? (tv.V - v0) : R;
    const int2* rows = tv.rowtab + ((i64)w * tv.V + v0);
    {   // the A rows of the vrows that have slots in this window -> LDS
      const int mine = g + l * G;   // lane l < RPG: the group's l-th vrow (a vrow behind the tile's last: no slots)
      int ey = 0, ar = 0;
      if (l < RPG && mine < nr) {
        ey = rows[mine].y;
        ar = tv.vr_row[v0 + mine];
      }
      // The A rows go from memory to LDS without passing through registers (the batch loop leaves none to hold RPG rows
      // in): a wave's four groups own four consecutive vrows, so its 64 lanes' 16 bytes are 1 KB in a row, which is the
      // form the LDS-writing load takes -- wave-uniform LDS base, lane x 16 B added by the hardware, per-lane source.
      float4* const wave_rows = lds + (threadIdx.x / kWave) * (kWave / L) * L;
      static_for<RPG>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const i64 arow = group_bcast<L, j>(ar);
        if (((unsigned)group_bcast<L, j>(ey) >> 16) != 0) ld16_to_lds(A + (arow * L + l) * 4, wave_rows + j * G * L);
      });
    }
    wait_vmem();       // this wave's A rows are in LDS
    __syncthreads();
    if (threadIdx.x >= NT - kWave) {   // the next task's part records, and its streams' lines into L2 (speed only)
      const int wn = task_sh[par ^ 1][0], tn = task_sh[par ^ 1][1];
      if (wn >= 0) {
        fetch_desc(par ^ 1, wn, tn);
        if (tv.touch) {
          const int4 nd = tv.tdesc[(i64)wn * tv.tiles + tn];
          const int lane = threadIdx.x & (kWave - 1);
          int tch[11];
#pragma unroll
          for (int q = 0; q < 11; ++q) tch[q] = 0;
          const int nrec = nd.y * 16;
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            const int at = (q * kWave + lane) * 64;
            if (at < nrec) tch[q] = tv.rec[(i64)nd.x * 16 + at];
          }
#pragma unroll
          for (int q = 0; q < 5; ++q) {
            const int at = (q * kWave + lane) * 32;
            if (at < nd.w) tch[3 + q] = tv.slotw[(i64)nd.z + at];
          }
          if (lane * 32 < nd.y) tch[8] = tv.bstart[nd.x + lane * 32];
          const int vn = tn * R;
          const int nrn = (tv.V - vn) < R ? (tv.V - vn) : R;
          if (lane * 16 < nrn) tch[9] = tv.rowtab[(i64)wn * tv.V + vn + lane * 16].x;
          if (lane * 32 < nrn) tch[10] = tv.vr_row[vn + lane * 32];
          // (waited for here, by this wave alone, so that the landing registers are free again in the batch loop)
          asm volatile("; touched %0 %1 %2 %3 %4 %5 %6 %7 %8 %9 %10" ::"v"(tch[0]), "v"(tch[1]), "v"(tch[2]), "v"(tch[3]),
                       "v"(tch[4]), "v"(tch[5]), "v"(tch[6]), "v"(tch[7]), "v"(tch[8]), "v"(tch[9]), "v"(tch[10]));
        }
      }
    }
    const unsigned win_id0 = (unsigned)w * (unsigned)tv.win_cols;
    const int p0 = desc_sh[par][0], p1 = desc_sh[par][1];
    for (int p = p0; p < p1; ++p) {
      int4 pt;
      if (p - p0 < kTileDescParts) {
        const int* d = &desc_sh[par][2 + 4 * (p - p0)];
        pt = make_int4(d[0], d[1], d[2], d[3]);
      } else {
        pt = tv.parts[p];
      }
      // (the same in every lane: kept in scalar registers across the batch loop)
      pt = make_int4(__builtin_amdgcn_readfirstlane(pt.x), __builtin_amdgcn_readfirstlane(pt.y),
                     __builtin_amdgcn_readfirstlane(pt.z), __builtin_amdgcn_readfirstlane(pt.w));
      const int nb = (pt.y + 15) >> 4;
      // batches come from the counter; the records of the batch after the one at hand are in flight behind its row requests
      int b = next_batch();
      int rw = 0, bs = 0;
      if (b < nb) { rw = tv.rec[((i64)pt.x + b) * 16 + l]; bs = tv.bstart[(i64)pt.x + b]; }
      while (b < nb) {
        const bool valid = b * 16 + l < pt.y;
        const int cnt = valid ? (rw & 3) + 1 : 0;
        const unsigned my_off = valid ? (win_id0 + (unsigned)(rw >> 2)) * 256u : 0u;
        const int first = bs + row16_incl_scan(cnt) - cnt;
        const int gmax = row16_max(cnt);
        int sw[4];   // (batches nearly always hold records of one slot count: a load no lane of the wave needs is not issued)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          sw[k] = 0;
          if (__builtin_amdgcn_ballot_w64(k < cnt) != 0 && k < cnt) sw[k] = tv.slotw[first + k];
        }
        float4 bb[16];
        static_for<16>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          const unsigned o = group_bcast<L, u>(my_off);
          bb[u] = ld16_off<float>(B, o + (unsigned)(l * 16));
        });
        const int bn = next_batch();
        if (bn < nb) { rw = tv.rec[((i64)pt.x + bn) * 16 + l]; bs = tv.bstart[(i64)pt.x + bn]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k < gmax) {   // group-uniform
            const unsigned my_koff = ((unsigned)sw[k] >> 16) * 256u;
            float part[16];
            static_for<16>([&](auto uc) {
              constexpr int u = decltype(uc)::value;
              const unsigned ko = group_bcast<L, u>(my_koff);
              const float4 av = *reinterpret_cast<const float4*>(lds_l + ko);
              part[u] = dot4(av, bb[u]);
            });
            const float r = group_dots_to_owner<L, 16>(part, l);
            if (k < cnt) res[sw[k] & 0xffff] = r;
          }
        }
        b = bn;
      }
      // the entries of the group's vrows of this part (pt.w <= R: at most RPG), one per lane, requested together; they
      // arrive while the group stands at the barrier
      int2 ent = make_int2(0, 0);
      if (l < RPG && g + l * G < pt.w) ent = rows[pt.z + g + l * G];
      __syncthreads();   // the part's results are in the buffer; every group has left the batch loop
      if (threadIdx.x == kWave) ctr_sh = 0;
      static_for<RPG>([&](auto kc) {   // every vrow's run -> y + its first edge id (no load here: no wait for stores)
        constexpr int k = decltype(kc)::value;
        const int first = group_bcast<L, k>(ent.x), ry = group_bcast<L, k>(ent.y);
        const int len = (int)((unsigned)ry >> 16), off = ry & 0xffff;
        for (int x = l; x < len; x += L) __builtin_nontemporal_store(res[off + x], y + ((i64)first + x));
      });
      if (p + 1 < p1) __syncthreads();   // the next part reuses the buffer and the counter
    }
    par ^= 1;
  }
}

}  // namespace graphop
