// Stand-alone program (its own main, no library code linked) that prints the launch geometry host_gat.h gives the GAT
// family, for tests/test_gat_host_layout.py to hold against the tests' own model of it.  One line per case:
//   cpg <n_cu> <G> <cap> <n_chunks> <gat_cpg> <gat_grid at that cpg>
//   row <n_cu> <cap> <n_chunks> <gat_cpg> <gat_grid at that cpg> <gat_row_pass cpg> <gat_row_pass n_blocks>
// host_gat.h reads the CU count and the knobs through tuning(), which the library defines next to its HIP state; here
// tuning() is this file's own object, so n_cu can be set and no device is needed.  Built with
// -fsanitize=address,undefined on the host side: the division by zero a cap <= 0 once led to would stop it.
#include <cstdio>

#include "host_gat.h"

namespace graphop {
static Tuning g_tuning;
const Tuning& tuning() { return g_tuning; }
}  // namespace graphop

using namespace graphop;

int main() {
  const i64 chunks[] = {0, 1, 15, 16, 17, 4095, 4096, 1000000, 8192 * 16 * 3 + 1};
  const int caps[] = {-1, 0, 1, 3, 16};
  for (int n_cu : {1, 256}) {
    g_tuning.n_cu = n_cu;
    for (int cap : caps)
      for (i64 n : chunks) {
        for (int G : {16, 32, 64}) {
          const int cpg = gat_cpg(n, cap, G);
          printf("cpg %d %d %d %lld %d %lld\n", n_cu, G, cap, (long long)n, cpg, (long long)gat_grid(n, cpg, G));
        }
        const int cpg = gat_cpg(n, cap);
        const GatRowPass geo = gat_row_pass(n, cap);
        printf("row %d %d %lld %d %lld %d %lld\n", n_cu, cap, (long long)n, cpg, (long long)gat_grid(n, cpg), geo.cpg,
               (long long)geo.n_blocks);
      }
  }
  return 0;
}
