// TILE layout of the window-owner tasks for the SDDMM-type tile driver (kernels_tile.h): host-side builder.
// Plain C++ (no HIP): plan.hip runs it on copies of a window structure's tables, tests/host/tile_layout_check.cpp runs it
// against a brute-force count.
//
// A task is (column window w, row tile t): the R consecutive vrows [t * R, (t + 1) * R) of the window structure inside
// window w, vrow v owning the slots [wp_lo[w * V + v], wp_hi[w * V + v]).  A task is cut into PARTS of consecutive vrows
// whose slots fit the kernel's LDS result buffer (`cap` floats; nearly always one part).  Inside a part the slots are
// GROUPED BY NEIGHBOUR ID: a group of c slots becomes c / 4 column records of 4 slots and one of c % 4, so that a lane
// group that holds 16 records never waits for a hub column; the part's records are ordered by slot count (4, 3, 2, 1),
// then by id -- 16 consecutive records (a BATCH) nearly always have the same count, so the lane groups of a wave, which
// run in lock step, finish a batch together.
//   rec[16 * batch + j]   16 bits: ((neighbour id - first id of the window) << 2) | (slots - 1); windows of at most
//                         16384 ids (4 MB of 256-B rows); the part's last batch is padded with zeros
//   bstart[batch]         index into slotw of the first slot word of the batch; the words of a batch's records follow
//                         each other in record order
//   slotw[...]            (row in tile << 16) | offset of the result in the part's result buffer
//   parts[p]              (first batch, records, first row in tile, rows)
//   part_ptr[w * tiles + t .. + 1]   the task's parts
//   tdesc[w * tiles + t]  (first batch, batches, first slot word, slot words) of the task
//   rowtab[w * V + v]     (first slot of the vrow in the window = edge id of its first result,
//                          offset of its run in the result buffer | slots << 16): a vrow's results are ONE run
#pragma once
#include <algorithm>
#include <cstdint>
#include <thread>
#include <vector>

namespace graphop {

constexpr int kTileMaxRows = 384;          // rows per tile the kernel is launched with: 128, 192, 256 or 384
constexpr int kTileMaxCap = 65535;         // result offsets are 16 bits
constexpr int kTileMaxRowSlots = 65535;    // ... and so is a vrow's slot count inside one window
constexpr int kTileRecSlots = 4;           // slots per column record
constexpr int kTileBatch = 16;             // records per batch = lanes of a lane group
constexpr int kTileMaxWinCols = 1 << 14;   // a column record is 16 bits: 14 of id inside the window, 2 of slot count
constexpr int kTileSlotPad = 64;           // ints behind the last slot word (a batch's loads never leave the array)

struct TileTotals {
  long long slots = 0, distinct = 0, records = 0, batches = 0, parts = 0;
  int max_part_slots = 0;
  bool fits = true;     // false: a vrow holds more slots inside one window than `cap` (no layout)
  double repeat_fraction() const { return slots > 0 ? 1.0 - (double)distinct / (double)slots : 0.0; }
};

struct TileLayoutHost {
  std::vector<int> part_ptr;   // [W * tiles + 1]
  std::vector<int> parts;      // [4 * n_parts]
  std::vector<uint16_t> rec;   // [16 * n_batches]
  std::vector<int> bstart;     // [n_batches]
  std::vector<int> slotw;      // [slots + kTileSlotPad]
  std::vector<int> rowtab;     // [2 * W * V]
  std::vector<int> tdesc;      // [4 * W * tiles]
  std::vector<long long> task_slots, task_distinct;   // [W * tiles] (checks and statistics)
};

namespace tile_detail {

struct Scratch {
  std::vector<int> cnt, pos4, posr, seen, touched;
  explicit Scratch(long long win_cols) : cnt((size_t)win_cols, 0), pos4((size_t)win_cols, 0), posr((size_t)win_cols, 0), seen((size_t)win_cols, 0) {}
};

struct TaskCount {
  int parts = 0;
  long long batches = 0, slots = 0, distinct = 0, records = 0;
  int max_part_slots = 0;
  bool fits = true;
};

struct Geometry {
  int V, W, R, cap, tiles;
  long long win_cols;
  const int *wp_lo, *wp_hi, *idx32;
};

// One task.  out == nullptr: count only.  Otherwise fill at (first part, first batch, first slot word) = (p0, b0, s0).
inline TaskCount do_task(const Geometry& g, int w, int t, Scratch& sc, TileLayoutHost* out, int p0, long long b0, long long s0) {
  TaskCount tc;
  const int v0 = t * g.R, nr = std::min(g.R, g.V - v0);
  const long long base = (long long)w * g.V + v0, col0 = (long long)w * g.win_cols;
  int i = 0;
  while (i < nr) {
    // rows of this part
    int i1 = i, part_slots = 0;
    while (i1 < nr) {
      const int len = g.wp_hi[base + i1] - g.wp_lo[base + i1];
      if (len > g.cap || len > kTileMaxRowSlots) { tc.fits = false; return tc; }
      if (part_slots + len > g.cap) break;
      part_slots += len;
      ++i1;
    }
    if (part_slots == 0) break;   // (then i1 == nr) only empty rows are left: no part of their own
    // group the part's slots by neighbour id
    sc.touched.clear();
    for (int r = i; r < i1; ++r)
      for (int e = g.wp_lo[base + r]; e < g.wp_hi[base + r]; ++e) {
        const int c = (int)(g.idx32[e] - col0);
        if (sc.cnt[(size_t)c]++ == 0) sc.touched.push_back(c);
      }
    std::sort(sc.touched.begin(), sc.touched.end());
    long long ncls[kTileRecSlots + 1] = {0, 0, 0, 0, 0};   // records of 1 .. 4 slots
    for (const int c : sc.touched) {
      const int n = sc.cnt[(size_t)c];
      ncls[kTileRecSlots] += n / kTileRecSlots;
      if (n % kTileRecSlots) ++ncls[n % kTileRecSlots];
    }
    const long long nrec = ncls[1] + ncls[2] + ncls[3] + ncls[4];
    const long long nbatch = (nrec + kTileBatch - 1) / kTileBatch;
    if (out) {
      // records in the order 4, 3, 2, 1 slots; rfirst / sfirst = first record / first slot word of every class
      long long rfirst[kTileRecSlots + 1], sfirst[kTileRecSlots + 1], rcur[kTileRecSlots + 1];
      long long racc = 0, sacc = 0;
      for (int k = kTileRecSlots; k >= 1; --k) { rfirst[k] = racc; sfirst[k] = sacc; racc += ncls[k]; sacc += ncls[k] * k; rcur[k] = 0; }
      uint16_t* rec = out->rec.data() + (b0 + tc.batches) * kTileBatch;
      for (long long q = 0; q < nbatch * kTileBatch; ++q) rec[q] = 0;
      for (const int c : sc.touched) {
        const int n = sc.cnt[(size_t)c], full = n / kTileRecSlots, rem = n % kTileRecSlots;
        sc.pos4[(size_t)c] = (int)(sfirst[kTileRecSlots] + rcur[kTileRecSlots] * kTileRecSlots);
        for (int q = 0; q < full; ++q) rec[rfirst[kTileRecSlots] + rcur[kTileRecSlots]++] = (uint16_t)((c << 2) | (kTileRecSlots - 1));
        if (rem) {
          sc.posr[(size_t)c] = (int)(sfirst[rem] + rcur[rem] * rem);
          rec[rfirst[rem] + rcur[rem]++] = (uint16_t)((c << 2) | (rem - 1));
        }
      }
      // first slot word of every batch: the records in front of it, class by class
      int* bstart = out->bstart.data() + (b0 + tc.batches);
      const long long sbase = s0 + tc.slots;
      for (long long b = 0; b < nbatch; ++b) {
        const long long q = b * kTileBatch;
        long long s = 0;
        for (int k = kTileRecSlots; k >= 1; --k) {
          const long long in_front = std::min(std::max(q - rfirst[k], 0LL), ncls[k]);
          s += in_front * k;
        }
        bstart[b] = (int)(sbase + s);
      }
      // slot words, and the rows' runs in the result buffer
      int off = 0;
      for (int r = i; r < i1; ++r) {
        const int lo = g.wp_lo[base + r], hi = g.wp_hi[base + r];
        out->rowtab[2 * (size_t)(base + r)] = lo;
        out->rowtab[2 * (size_t)(base + r) + 1] = (int)((unsigned)off | ((unsigned)(hi - lo) << 16));
        for (int e = lo; e < hi; ++e) {
          const int c = (int)(g.idx32[e] - col0);
          const int k = sc.seen[(size_t)c]++;
          const int n4 = (sc.cnt[(size_t)c] / kTileRecSlots) * kTileRecSlots;
          const int pos = k < n4 ? sc.pos4[(size_t)c] + k : sc.posr[(size_t)c] + (k - n4);
          out->slotw[(size_t)(sbase + pos)] = (r << 16) | (off + (e - lo));
        }
        off += hi - lo;
      }
      int* pt = out->parts.data() + 4 * (size_t)(p0 + tc.parts);
      pt[0] = (int)(b0 + tc.batches); pt[1] = (int)nrec; pt[2] = i; pt[3] = i1 - i;
    }
    for (const int c : sc.touched) { sc.cnt[(size_t)c] = 0; sc.seen[(size_t)c] = 0; }
    tc.parts += 1;
    tc.batches += nbatch;
    tc.slots += part_slots;
    tc.distinct += (long long)sc.touched.size();
    tc.records += nrec;
    tc.max_part_slots = std::max(tc.max_part_slots, part_slots);
    i = i1;
  }
  if (out) {
    // rows behind the last part (empty ones): defined, empty runs
    const int done = tc.parts > 0 ? out->parts[4 * (size_t)(p0 + tc.parts - 1) + 2] + out->parts[4 * (size_t)(p0 + tc.parts - 1) + 3] : 0;
    for (int r = done; r < nr; ++r) {
      out->rowtab[2 * (size_t)(base + r)] = g.wp_lo[base + r];
      out->rowtab[2 * (size_t)(base + r) + 1] = 0;
    }
  }
  return tc;
}

template <typename F>
inline void parallel_tasks(long long n, int threads, F&& f) {
  if (threads < 1) threads = 1;
  if (threads > n) threads = (int)(n > 0 ? n : 1);
  if (threads == 1) { f(0, 0LL, n); return; }
  std::vector<std::thread> pool;
  for (int k = 0; k < threads; ++k) pool.emplace_back([&f, k, n, threads]() { f(k, n * k / threads, n * (k + 1) / threads); });
  for (auto& th : pool) th.join();
}

}  // namespace tile_detail

// Count (out == nullptr) or count and build the layout of a window structure for tiles of R vrows and result buffers of
// `cap` floats.  wp_lo / wp_hi: [W * V], idx32: the neighbour ids per slot (ascending inside a row), win_cols: ids per
// window.  Returns the totals; totals.fits == false leaves `out` unspecified.
inline TileTotals build_tile_layout(int V, int W, int R, int cap, long long win_cols, const int* wp_lo, const int* wp_hi,
                                    const int* idx32, TileLayoutHost* out, int threads = 0,
                                    std::vector<tile_detail::TaskCount>* reuse = nullptr) {
  using namespace tile_detail;
  TileTotals tot;
  if (V < 1 || W < 1 || R < 1 || R > kTileMaxRows || cap < 1 || cap > kTileMaxCap || win_cols < 1 || win_cols > kTileMaxWinCols) { tot.fits = false; return tot; }
  const int tiles = (V + R - 1) / R;
  const long long ntask = (long long)W * tiles;
  const Geometry g{V, W, R, cap, tiles, win_cols, wp_lo, wp_hi, idx32};
  if (threads <= 0) {
    const unsigned hw = std::thread::hardware_concurrency();
    threads = (int)std::min<unsigned>(hw ? hw : 1, 16);
  }
  // `reuse`: the per-task counts of an earlier call with the same arguments (filled here when empty): a caller that
  // counts first and builds afterwards walks the slots twice, not three times
  std::vector<TaskCount> local;
  std::vector<TaskCount>& counts = reuse ? *reuse : local;
  if ((long long)counts.size() != ntask) {
    counts.assign((size_t)ntask, TaskCount());
    parallel_tasks(ntask, threads, [&](int, long long a, long long b) {
      Scratch sc(win_cols);
      for (long long k = a; k < b; ++k) counts[(size_t)k] = do_task(g, (int)(k / tiles), (int)(k % tiles), sc, nullptr, 0, 0, 0);
    });
  }
  std::vector<long long> b0((size_t)ntask + 1, 0), s0((size_t)ntask + 1, 0);
  std::vector<int> p0((size_t)ntask + 1, 0);
  for (long long k = 0; k < ntask; ++k) {
    const TaskCount& c = counts[(size_t)k];
    tot.fits = tot.fits && c.fits;
    tot.slots += c.slots; tot.distinct += c.distinct; tot.records += c.records; tot.batches += c.batches; tot.parts += c.parts;
    tot.max_part_slots = std::max(tot.max_part_slots, c.max_part_slots);
    p0[(size_t)k + 1] = p0[(size_t)k] + c.parts;
    b0[(size_t)k + 1] = b0[(size_t)k] + c.batches;
    s0[(size_t)k + 1] = s0[(size_t)k] + c.slots;
  }
  if (!tot.fits || !out) return tot;
  if (tot.slots + kTileSlotPad >= 0x7fffffffLL || tot.batches * kTileBatch >= 0x7fffffffLL) { tot.fits = false; return tot; }
  out->part_ptr.assign(p0.begin(), p0.end());
  out->parts.assign(4 * (size_t)tot.parts, 0);
  out->rec.assign((size_t)(tot.batches * kTileBatch), 0);
  out->bstart.assign((size_t)tot.batches, 0);
  out->slotw.assign((size_t)(tot.slots + kTileSlotPad), 0);
  out->rowtab.assign(2 * (size_t)W * V, 0);
  out->tdesc.assign(4 * (size_t)ntask, 0);
  out->task_slots.resize((size_t)ntask);
  out->task_distinct.resize((size_t)ntask);
  for (long long k = 0; k < ntask; ++k) {
    out->task_slots[(size_t)k] = counts[(size_t)k].slots;
    out->task_distinct[(size_t)k] = counts[(size_t)k].distinct;
    int* td = out->tdesc.data() + 4 * (size_t)k;
    td[0] = (int)b0[(size_t)k]; td[1] = (int)counts[(size_t)k].batches; td[2] = (int)s0[(size_t)k]; td[3] = (int)counts[(size_t)k].slots;
  }
  parallel_tasks(ntask, threads, [&](int, long long a, long long b) {
    Scratch sc(win_cols);
    for (long long k = a; k < b; ++k)
      (void)do_task(g, (int)(k / tiles), (int)(k % tiles), sc, out, p0[(size_t)k], b0[(size_t)k], s0[(size_t)k]);
  });
  return tot;
}

}  // namespace graphop
