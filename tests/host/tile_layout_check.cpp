// Stand-alone check of the tile layout builder (custom_op_benchmark_amd/csrc/tile_layout.h) against brute force, on the
// CPU: tests/test_sddmm_tile_host.py compiles and runs it (with the address and undefined-behaviour sanitizers).
//   tile_layout_check                      random graphs: exit status 0 and "ok" when every check holds
//   tile_layout_check FILE N_COLS T W R CAP   statistics of the layout of the CSR in FILE (int64 n_rows, int64 indptr[n_rows + 1],
//                                          int32 indices[...]; ids ascending inside a row) -- no checks beyond the totals
// Checked per graph and geometry:
//   - slots and distinct neighbours of every (window, tile) task equal a brute-force count over the window tables;
//   - every column record has 1 .. 4 slots, the records of a part are ordered by slot count (descending);
//   - replaying the kernel's index arithmetic (batch -> records -> slot words -> result buffer -> the rows' runs -> y)
//     writes every edge id exactly once, with the pair (row of the vrow, neighbour id) that owns the slot, and never
//     reads or writes outside an array or the result buffer; a vrow's results are one contiguous run.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "tile_layout.h"

using namespace graphop;

struct Csr {
  int n_rows = 0, n_cols = 0;
  std::vector<long long> indptr;
  std::vector<int> idx;
};

// window tables as plan.hip builds them (k_sweep_row_windows, k_sweep_fill): rows longer than T slots are cut into P
// pieces, piece p takes the p-th 1/P of the row's slots inside every window
struct Tables {
  int V = 0, W = 0;
  long long win_cols = 0;
  std::vector<int> vr_row, wp_lo, wp_hi;
};
static Tables make_tables(const Csr& g, int W, int T) {
  Tables t;
  t.W = W;
  t.win_cols = (g.n_cols + W - 1) / W;
  std::vector<int> seg_row, first_v;
  for (int r = 0; r < g.n_rows; ++r) {
    const long long len = g.indptr[r + 1] - g.indptr[r];
    if (len == 0) continue;
    seg_row.push_back(r);
    first_v.push_back(t.V);
    t.V += (int)((len + T - 1) / T);
  }
  first_v.push_back(t.V);
  t.vr_row.assign(t.V, 0);
  t.wp_lo.assign((size_t)t.V * W, 0);
  t.wp_hi.assign((size_t)t.V * W, 0);
  for (size_t s = 0; s < seg_row.size(); ++s) {
    const int r = seg_row[s];
    const long long e0 = g.indptr[r], e1 = g.indptr[r + 1];
    const int P = first_v[s + 1] - first_v[s];
    std::vector<long long> rw(W + 1);
    for (int w = 0; w <= W; ++w) {
      if (w == 0) rw[w] = e0;
      else if (w == W) rw[w] = e1;
      else rw[w] = std::lower_bound(g.idx.begin() + e0, g.idx.begin() + e1, (int)(w * t.win_cols)) - g.idx.begin();
    }
    for (int p = 0; p < P; ++p) {
      const int v = first_v[s] + p;
      t.vr_row[v] = r;
      for (int w = 0; w < W; ++w) {
        const long long a = rw[w], len = rw[w + 1] - a, q = (len + P - 1) / P;
        t.wp_lo[(size_t)w * t.V + v] = (int)(a + std::min<long long>((long long)p * q, len));
        t.wp_hi[(size_t)w * t.V + v] = (int)(a + std::min<long long>((long long)(p + 1) * q, len));
      }
    }
  }
  return t;
}

static Csr random_graph(std::mt19937& rng, int n_rows, int n_cols, int n_edges, bool hub_col, int hub_row_slots, double empty) {
  Csr g;
  g.n_rows = n_rows; g.n_cols = n_cols;
  std::vector<std::set<int>> rows(n_rows);
  std::uniform_int_distribution<int> rr(0, n_rows - 1), cc(0, n_cols - 1);
  std::vector<char> is_empty(n_rows, 0);
  for (int r = 0; r < n_rows; ++r) is_empty[r] = std::uniform_real_distribution<double>(0, 1)(rng) < empty;
  for (int k = 0; k < n_edges; ++k) {
    // skewed columns: half of the draws fall into the first sixteenth of the ids (repeats inside a tile)
    int c = cc(rng);
    if (k & 1) c /= 16;
    const int r = rr(rng);
    if (!is_empty[r]) rows[r].insert(c);
  }
  if (hub_col) for (int r = 0; r < n_rows; ++r) if (!is_empty[r]) rows[r].insert(n_cols / 3);
  if (hub_row_slots > 0) while ((int)rows[n_rows / 2].size() < std::min(hub_row_slots, n_cols)) rows[n_rows / 2].insert(cc(rng));
  g.indptr.push_back(0);
  for (int r = 0; r < n_rows; ++r) {
    for (int c : rows[r]) g.idx.push_back(c);
    g.indptr.push_back((long long)g.idx.size());
  }
  return g;
}

#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                        \
      fprintf(stderr, "\n");                               \
      return false;                                        \
    }                                                      \
  } while (0)

static bool check(const Csr& g, const Tables& t, int R, int cap, const char* what) {
  const long long E = (long long)g.idx.size();
  TileLayoutHost lay;
  // count, then fill from the kept counts (as plan.hip does), and once more in one call: the same layout
  std::vector<tile_detail::TaskCount> counts;
  const TileTotals cnt = build_tile_layout(t.V, t.W, R, cap, t.win_cols, t.wp_lo.data(), t.wp_hi.data(), g.idx.data(), nullptr, 3, &counts);
  const TileTotals tot = build_tile_layout(t.V, t.W, R, cap, t.win_cols, t.wp_lo.data(), t.wp_hi.data(), g.idx.data(), &lay, 3, &counts);
  {
    TileLayoutHost one;
    const TileTotals t1 = build_tile_layout(t.V, t.W, R, cap, t.win_cols, t.wp_lo.data(), t.wp_hi.data(), g.idx.data(), &one, 2);
    CHECK(t1.slots == tot.slots && one.rec == lay.rec && one.slotw == lay.slotw && one.bstart == lay.bstart && one.parts == lay.parts &&
          one.rowtab == lay.rowtab && one.tdesc == lay.tdesc && one.part_ptr == lay.part_ptr, "%s: reused counts give another layout", what);
  }
  CHECK(cnt.fits && tot.fits, "%s: does not fit", what);
  CHECK(cnt.slots == tot.slots && cnt.distinct == tot.distinct && cnt.records == tot.records, "%s: count and fill disagree", what);
  CHECK(tot.slots == E, "%s: %lld slots, %lld edges", what, tot.slots, E);
  CHECK(tot.max_part_slots <= cap, "%s: part of %d slots", what, tot.max_part_slots);
  const int tiles = (t.V + R - 1) / R;
  CHECK((long long)lay.part_ptr.size() == (long long)t.W * tiles + 1, "%s: part_ptr size", what);
  CHECK((long long)lay.slotw.size() == E + kTileSlotPad, "%s: slotw size", what);
  std::vector<char> y_written((size_t)E, 0);
  long long distinct_sum = 0, rec_sum = 0;
  for (int w = 0; w < t.W; ++w)
    for (int tt = 0; tt < tiles; ++tt) {
      const long long task = (long long)w * tiles + tt;
      const int v0 = tt * R, nr = std::min(R, t.V - v0);
      // brute force
      std::set<int> ids;
      long long slots = 0;
      for (int i = 0; i < nr; ++i)
        for (int e = t.wp_lo[(size_t)w * t.V + v0 + i]; e < t.wp_hi[(size_t)w * t.V + v0 + i]; ++e) { ids.insert(g.idx[e]); ++slots; }
      CHECK(lay.task_slots[task] == slots, "%s: task (%d, %d): %lld slots, brute force %lld", what, w, tt, lay.task_slots[task], slots);
      CHECK(lay.tdesc[4 * task + 3] == slots, "%s: tdesc slots", what);
      // the layout counts distinct ids per PART; with one part that is the task's count
      const int p0 = lay.part_ptr[task], p1 = lay.part_ptr[task + 1];
      CHECK(p0 <= p1 && p1 * 4 <= (int)lay.parts.size(), "%s: part_ptr", what);
      if (p1 - p0 <= 1) CHECK(lay.task_distinct[task] == (long long)ids.size(), "%s: task (%d, %d): %lld distinct, brute force %zu", what, w, tt, lay.task_distinct[task], ids.size());
      else CHECK(lay.task_distinct[task] >= (long long)ids.size(), "%s: distinct below the brute-force count", what);
      distinct_sum += lay.task_distinct[task];
      int next_row = 0;
      long long task_batches = 0;
      for (int p = p0; p < p1; ++p) {
        const int* pt = &lay.parts[4 * (size_t)p];
        const int batch0 = pt[0], nrec = pt[1], row0 = pt[2], nrows = pt[3];
        CHECK(row0 >= next_row && row0 + nrows <= nr && nrows > 0, "%s: part rows", what);
        for (int i = next_row; i < row0; ++i) CHECK(t.wp_hi[(size_t)w * t.V + v0 + i] == t.wp_lo[(size_t)w * t.V + v0 + i], "%s: skipped row has slots", what);
        next_row = row0 + nrows;
        if (p == p0) CHECK(lay.tdesc[4 * task] == batch0, "%s: tdesc first batch", what);
        // the rows' runs: disjoint, in order, inside the buffer
        int expect_off = 0;
        for (int i = row0; i < row0 + nrows; ++i) {
          const size_t at = (size_t)w * t.V + v0 + i;
          const int lo = lay.rowtab[2 * at];
          const unsigned packed = (unsigned)lay.rowtab[2 * at + 1];
          CHECK(lo == t.wp_lo[at] && (int)(packed >> 16) == t.wp_hi[at] - t.wp_lo[at], "%s: rowtab", what);
          CHECK((int)(packed & 0xffff) == expect_off, "%s: run offsets", what);
          expect_off += (int)(packed >> 16);
        }
        CHECK(expect_off <= cap, "%s: buffer overflow", what);
        std::vector<int> res_id((size_t)expect_off, -1), res_row((size_t)expect_off, -1);
        const int nb = (nrec + 15) / 16;
        task_batches += nb;
        int prev_cnt = kTileRecSlots;
        for (int b = 0; b < nb; ++b) {
          const long long gb = (long long)batch0 + b;
          CHECK(gb < (long long)lay.bstart.size() && (gb + 1) * 16 <= (long long)lay.rec.size(), "%s: batch index", what);
          int at = lay.bstart[gb];
          if (p == p0 && b == 0) CHECK(lay.tdesc[4 * task + 2] == at, "%s: tdesc first slot word", what);
          for (int l = 0; l < 16; ++l) {
            if (b * 16 + l >= nrec) { CHECK(lay.rec[gb * 16 + l] == 0, "%s: padding record", what); continue; }
            const int rw = lay.rec[gb * 16 + l], c = (rw & 3) + 1, id = (int)(w * t.win_cols) + (rw >> 2);
            CHECK(c <= prev_cnt, "%s: records not ordered by slot count", what);
            prev_cnt = c;
            CHECK(id >= (long long)w * t.win_cols && id < (long long)(w + 1) * t.win_cols && id < g.n_cols, "%s: id outside the window", what);
            for (int k = 0; k < c; ++k, ++at) {
              CHECK(at >= 0 && at < E, "%s: slot word index", what);
              const unsigned sw = (unsigned)lay.slotw[at];
              const int r = (int)(sw >> 16), off = (int)(sw & 0xffff);
              CHECK(r >= row0 && r < row0 + nrows, "%s: slot row outside the part", what);
              CHECK(off < expect_off && res_id[off] < 0, "%s: result offset written twice or outside", what);
              res_id[off] = id;
              res_row[off] = r;
            }
          }
        }
        rec_sum += nrec;
        for (int i = row0; i < row0 + nrows; ++i) {   // the flush
          const size_t at = (size_t)w * t.V + v0 + i;
          const int lo = lay.rowtab[2 * at];
          const unsigned packed = (unsigned)lay.rowtab[2 * at + 1];
          for (int x = 0; x < (int)(packed >> 16); ++x) {
            const int off = (int)(packed & 0xffff) + x;
            CHECK(lo + x >= 0 && lo + x < E && !y_written[lo + x], "%s: edge %d written twice", what, lo + x);
            y_written[lo + x] = 1;
            CHECK(res_id[off] == g.idx[lo + x] && res_row[off] == i, "%s: edge %d got (row %d, id %d), wants (row %d, id %d)", what, lo + x,
                  res_row[off], res_id[off], i, g.idx[lo + x]);
            CHECK(g.indptr[t.vr_row[v0 + i]] <= lo + x && lo + x < g.indptr[t.vr_row[v0 + i] + 1], "%s: edge not of the vrow's row", what);
          }
        }
      }
      for (int i = next_row; i < nr; ++i) {
        const size_t at = (size_t)w * t.V + v0 + i;
        CHECK(t.wp_hi[at] == t.wp_lo[at] && ((unsigned)lay.rowtab[2 * at + 1] >> 16) == 0, "%s: trailing row has slots", what);
      }
      CHECK(lay.tdesc[4 * task + 1] == task_batches, "%s: tdesc batches", what);
    }
  for (long long e = 0; e < E; ++e) CHECK(y_written[e], "%s: edge %lld never written", what, e);
  CHECK(distinct_sum == tot.distinct && rec_sum == tot.records, "%s: totals", what);
  printf("  %-44s V %5d W %3d R %3d cap %5d: slots %7lld distinct %7lld (repeats %4.1f %%) records %7lld parts %lld\n", what, t.V, t.W, R,
         cap, tot.slots, tot.distinct, 100.0 * tot.repeat_fraction(), tot.records, tot.parts);
  return true;
}

static int stats_of_file(int argc, char** argv) {
  if (argc < 7) { fprintf(stderr, "usage: %s FILE N_COLS T W R CAP\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  Csr g;
  long long n_rows = 0;
  if (fread(&n_rows, 8, 1, f) != 1) return 2;
  g.n_rows = (int)n_rows;
  g.n_cols = atoi(argv[2]);
  g.indptr.resize((size_t)n_rows + 1);
  if (fread(g.indptr.data(), 8, (size_t)n_rows + 1, f) != (size_t)n_rows + 1) return 2;
  g.idx.resize((size_t)g.indptr.back());
  if (fread(g.idx.data(), 4, g.idx.size(), f) != g.idx.size()) return 2;
  fclose(f);
  const int T = atoi(argv[3]), W = atoi(argv[4]);
  const Tables t = make_tables(g, W, T);
  for (int a = 5; a + 1 < argc; a += 2) {
    const int R = atoi(argv[a]), cap = atoi(argv[a + 1]);
    TileLayoutHost lay;
    const TileTotals tot = build_tile_layout(t.V, t.W, R, cap, t.win_cols, t.wp_lo.data(), t.wp_hi.data(), g.idx.data(), &lay);
    const double bytes = 2.0 * lay.rec.size() + 4.0 * (lay.part_ptr.size() + lay.parts.size() + lay.bstart.size() + lay.slotw.size() + lay.rowtab.size() + lay.tdesc.size());
    printf("R %d cap %d: fits %d V %d tasks %lld parts %lld slots %lld distinct %lld repeats %.2f %% records %lld batches %lld "
           "(%.3f per 16 slots) max part %d layout %.1f MiB (%.2f B per slot)\n", R, cap, (int)tot.fits, t.V, (long long)t.W * ((t.V + R - 1) / R),
           tot.parts, tot.slots, tot.distinct, 100.0 * tot.repeat_fraction(), tot.records, tot.batches,
           16.0 * tot.batches / (double)tot.slots, tot.max_part_slots, bytes / 1048576.0, bytes / (double)tot.slots);
    long long by_cnt[5] = {0, 0, 0, 0, 0};
    for (long long q = 0; q < (long long)lay.rec.size(); ++q) by_cnt[(lay.rec[q] & 3) + 1]++;
    printf("   records (incl. padding) by slots: 1: %lld  2: %lld  3: %lld  4: %lld\n", by_cnt[1], by_cnt[2], by_cnt[3], by_cnt[4]);
    fflush(stdout);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1) return stats_of_file(argc, argv);
  std::mt19937 rng(12345);
  bool ok = true;
  struct Case { const char* name; int n_rows, n_cols, E; bool hub_col; int hub_row; double empty; int W, T, R, cap; };
  const Case cases[] = {
      {"700 x 700, ragged last tile", 700, 700, 20000, false, 0, 0.0, 8, 64, 128, 11000},
      {"700 x 700, hub column", 700, 700, 20000, true, 0, 0.0, 8, 64, 128, 11000},
      {"700 x 5400, hub row of 5000 slots (pieces)", 700, 5400, 20000, false, 5000, 0.0, 8, 64, 128, 11000},
      {"30 % empty rows", 700, 700, 6000, false, 0, 0.3, 16, 64, 128, 11000},
      {"300 x 900", 300, 900, 9000, false, 0, 0.0, 4, 64, 192, 7000},
      {"900 x 300", 900, 300, 9001, true, 0, 0.0, 4, 64, 256, 20000},
      {"small buffer: several parts per task", 700, 700, 20000, true, 0, 0.0, 2, 64, 384, 700},
      {"one window, one tile", 100, 50, 777, true, 0, 0.1, 1, 4096, 384, 15000},
      {"rows longer than the buffer allows pieces of", 64, 4000, 30000, false, 3000, 0.0, 2, 1024, 128, 1024},
  };
  for (const Case& c : cases) {
    const Csr g = random_graph(rng, c.n_rows, c.n_cols, c.E, c.hub_col, c.hub_row, c.empty);
    const Tables t = make_tables(g, c.W, c.T);
    ok = check(g, t, c.R, c.cap, c.name) && ok;
  }
  // a vrow that does not fit the buffer: reported, not built
  {
    const Csr g = random_graph(rng, 10, 3000, 100, false, 2000, 0.0);
    const Tables t = make_tables(g, 1, 4096);
    const TileTotals tot = build_tile_layout(t.V, t.W, 128, 1000, t.win_cols, t.wp_lo.data(), t.wp_hi.data(), g.idx.data(), nullptr, 2);
    if (tot.fits) { fprintf(stderr, "FAILED: a vrow of 2000 slots fits a buffer of 1000\n"); ok = false; }
  }
  printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
