"""Graphs for the tile driver's tests (tests/test_sddmm_tile.py), and what can be said about their tile layout from the
edge list alone: which column window an edge falls into, the offset bits of its column record, how many parts a (window,
tile) task is cut into while no row is cut.  Imports without a GPU; nothing here reads the layout the plan builds."""
import numpy as np
import torch

from custom_op_benchmark_amd import graphs

# floats of the LDS result buffer per tile height (csrc/graphop_hip.hip: choose_tile -- 158 KiB for the workgroups of a CU,
# two of them up to 192 rows, rounded down to 256 B, less the tile's A rows of 256 B)
TILE_LDS_BYTES = 158 * 1024


def tile_cap(rows):
    per_cu = 2 if rows <= 192 else 1
    return ((TILE_LDS_BYTES // per_cu) & ~255) // 4 - rows * 64


DESC_PARTS = 4          # kernels_tile.h: kTileDescParts, the parts of a task handed over through LDS
MAX_WIN_COLS = 1 << 14  # tile_layout.h: kTileMaxWinCols


def dense_rows_graph(n_src, n_dst, per_row, seed, lo_share=None, chunk_size=32):
    """Every row draws per_row columns uniformly with replacement (duplicate (row, column) pairs stay: they land in records
    of several slots).  lo_share: that share of a row's draws comes from the lower half of the columns, the rest from
    the upper half (None: uniform over all columns)."""
    gen = torch.Generator().manual_seed(seed)
    src = torch.arange(n_src).repeat_interleave(per_row)
    if lo_share is None:
        dst = torch.randint(0, n_dst, (n_src * per_row,), generator=gen)
    else:
        half, n_lo = n_dst // 2, int(round(per_row * lo_share))
        lo = torch.randint(0, half, (n_src, n_lo), generator=gen)
        hi = torch.randint(half, n_dst, (n_src, per_row - n_lo), generator=gen)
        dst = torch.cat([lo, hi], 1).reshape(-1)
    return graphs.graph_from_coo(src, dst, n_src, n_dst, chunk_size)


def full_width_graph(n_src, n_dst, n_edges, W, seed, chunk_size=32):
    """Uniform edges, plus, from a few rows spread over the graph, edges into the first id, the last id, the id whose
    offset has every bit set and the two ids of alternating offset bits of every one of the W windows of
    ceil(n_dst / W) ids (where the table has them)."""
    gen = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n_src, (n_edges,), generator=gen)
    dst = torch.randint(0, n_dst, (n_edges,), generator=gen)
    win_cols = -(-n_dst // W)
    ids = []
    for w in range(W):
        for off in (0, win_cols - 1, MAX_WIN_COLS - 1, 0x2AAA, 0x1555):
            c = w * win_cols + off
            if off < win_cols and c < n_dst:
                ids.append(c)
    ids = torch.tensor(sorted(set(ids)))
    rows = torch.tensor([0, 1, n_src // 3, n_src // 2, n_src - 1])
    es, ed = torch.meshgrid(rows, ids, indexing="ij")
    return graphs.graph_from_coo(torch.cat([src, es.reshape(-1)]), torch.cat([dst, ed.reshape(-1)]), n_src, n_dst, chunk_size)


def pooled_graph(n_src, n_dst, per_row, tile_rows, pool, seed, chunk_size=32):
    """Every row has exactly per_row edges; the rows [t * tile_rows, (t + 1) * tile_rows) draw them from a pool of `pool`
    columns of their own (drawn over the whole table), so nearly every slot of a tile repeats a neighbour of its tile."""
    gen = torch.Generator().manual_seed(seed)
    tiles = -(-n_src // tile_rows)
    pools = torch.randint(0, n_dst, (tiles, pool), generator=gen)
    pick = torch.randint(0, pool, (n_src, per_row), generator=gen)
    tile_of = torch.arange(n_src) // tile_rows
    dst = pools[tile_of.unsqueeze(1), pick].reshape(-1)
    src = torch.arange(n_src).repeat_interleave(per_row)
    return graphs.graph_from_coo(src, dst, n_src, n_dst, chunk_size)


def repeated_pair_graph(n_src, n_dst, n_edges, row, column, times, seed, chunk_size=32):
    """Uniform edges plus `times` copies of the edge (row, column)."""
    gen = torch.Generator().manual_seed(seed)
    src = torch.cat([torch.randint(0, n_src, (n_edges,), generator=gen), torch.full((times,), row)])
    dst = torch.cat([torch.randint(0, n_dst, (n_edges,), generator=gen), torch.full((times,), column)])
    return graphs.graph_from_coo(src, dst, n_src, n_dst, chunk_size)


def record_offsets(g, W):
    """-> (window, offset inside the window) of every edge's column, for W windows of ceil(n_dst / W) ids."""
    win_cols = -(-g.n_dst // W)
    dst = g.dst.numpy()
    return dst // win_cols, dst % win_cols


def task_parts_uncut(g, W, rows, cap):
    """-> [W, tiles] number of parts of every (window, tile) task, restated from the edge list for a graph in which
    every row has an edge and NO ROW IS CUT (vrow_t >= the longest row): the vrows then are the rows, a tile is `rows`
    consecutive ones, and a task is cut greedily into runs of whole rows of at most `cap` slots (csrc/tile_layout.h:
    do_task).  None where a row holds more than cap slots inside one window (no layout)."""
    deg = np.bincount(g.src.numpy(), minlength=g.n_src)
    assert deg.min() > 0
    w, _ = record_offsets(g, W)
    cnt = np.zeros((W, g.n_src), dtype=np.int64)
    np.add.at(cnt, (w, g.src.numpy()), 1)
    if cnt.max() > cap:
        return None
    tiles = -(-g.n_src // rows)
    out = np.zeros((W, tiles), dtype=np.int64)
    for wi in range(W):
        for t in range(tiles):
            c = cnt[wi, t * rows:(t + 1) * rows]
            i, parts = 0, 0
            while i < len(c):
                acc, j = 0, i
                while j < len(c) and acc + c[j] <= cap:
                    acc += c[j]
                    j += 1
                if acc == 0:
                    break
                parts, i = parts + 1, j
            out[wi, t] = parts
    return out
