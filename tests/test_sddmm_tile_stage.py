"""Staging and write-out of the tile driver of the SDDMM-type passes (csrc/kernels_tile.h): a lane group loads the
row-table entries of its R / G vrows in one round trip, requests their A rows together under the "has slots in this window"
predicate; for the write-out of a part it requests the entries of its vrows of that part together, one per lane, and then
stores run after run with no load in between.  (G = lane groups
per workgroup: 32 at 128 / 192 rows per tile, 64 at 256 / 384.)

Every case runs both passes through the C ABI into outputs full of NaN between guard bands, compares them with the
oracle at the bounds of tests/test_hip_parity.py and bit for bit with the window-owner strips (sddmm_tile = 0) under the
same window knobs, and proves from the edge list or the plan's info record that it reached the path it names.  The
result buffer's size comes from the library (graphop_sddmm_tile_cap), never from a literal here."""
import functools

import numpy as np
import pytest
import torch

from custom_op_benchmark_amd import _lib, graphs
from sddmm_tile_graphs import dense_rows_graph, record_offsets, task_parts_uncut
from test_hip_parity import close
from test_sddmm_tile import D, FORCED, GUARD, STRIPS, TAGS, TILE, graph_case, kernels_by_tag, knobs, run_case, sweeps_of
from util import random_graph

pytestmark = pytest.mark.gpu

GROUPS = {128: 32, 192: 32, 256: 64, 384: 64}   # lane groups per workgroup (512 / 1024 threads, 16 lanes each)
WIN_IDS = 128                                    # ids per window under window_kb = 32 (256-B rows)


def cap_of(rows):
    cap = int(_lib.lib().graphop_sddmm_tile_cap(rows))
    assert 0 < cap < 65536
    return cap


def tile_passes_into_poison(c, dev):
    """Both passes through the C ABI into views of E floats inside buffers full of NaN (test_sddmm_tile.py:
    passes_into, which keeps the plan to itself) -> (s, da, {tag: kernel}, the row-major plan).  Guard bands still NaN,
    no NaN inside, both results at the oracle's bound."""
    a8d = tuple(x.to(dev) for x in c.a8)
    Qd, Kd, Vd, dOd, ad = (x.to(dev) for x in (c.Q, c.K, c.V, c.dO, c.a))
    l, P = _lib.lib(), _lib.ptr
    plan_r, plan_c = _lib.get_plan(*a8d[:4], c.n_dst), _lib.get_plan(*a8d[4:], c.n_src)
    st = _lib.stream_of(Qd)
    dx = torch.empty_like(Vd)
    bufs = [torch.full((c.n_edges + 2 * GUARD,), float("nan"), device=dev) for _ in range(2)]
    y_s, y_da = (b[GUARD:GUARD + c.n_edges] for b in bufs)
    assert y_s.data_ptr() % 16 == 0 and y_da.data_ptr() % 16 == 0

    def step():
        _lib.check(l.graphop_maskedmm_csr_forward(_lib.F32, *(P(x) for x in a8d[:4]), P(Qd), P(Kd), P(y_s), a8d[0].numel(),
                                                  c.n_edges, c.n_src, c.n_dst, 1, D, plan_r.handle, st))
        _lib.check(l.graphop_vector_spmm_backward(_lib.F32, *(P(x) for x in a8d), P(ad), P(dOd), P(Vd), P(y_da), P(dx),
                                                  a8d[0].numel(), a8d[4].numel(), c.n_edges, c.n_dst, c.n_src, 1, D,
                                                  plan_r.handle, plan_c.handle, st))
    kern = kernels_by_tag(step)
    for b, v, want in zip(bufs, (y_s, y_da), (c.want_s, c.want_da)):
        assert bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[GUARD + c.n_edges:]).all())
        assert not bool(torch.isnan(v).any())
        close(v, want)
    return y_s.clone(), y_da.clone(), kern, plan_r


def check_stage(c, dev, prove=None, **kn):
    """The tile kernel on both tags into poisoned outputs against the oracle, prove(info, plan) under the same knobs, then the
    strips under the same window knobs: torch.equal on both results."""
    with knobs(**dict(FORCED, **kn)):
        s_t, da_t, kern, plan = tile_passes_into_poison(c, dev)
        assert [kern[t] for t in TAGS] == [TILE, TILE], kern
        info = plan.refresh_info()
        assert info.sddmm_tile_rows == kn.get("sddmm_tile_rows", FORCED["sddmm_tile_rows"]) and info.sddmm_tile_max_parts >= 1
        if prove:
            prove(info, plan)
    with knobs(**dict(dict(FORCED, **kn), sddmm_tile=0)):
        s_s, da_s, kern, _ = run_case(c, dev)
        assert [kern[t] for t in TAGS] == [STRIPS, STRIPS], kern
    close(s_s, c.want_s)
    close(da_s, c.want_da)
    assert torch.equal(s_t, s_s), "s"
    assert torch.equal(da_t, da_s), "da"


def window_counts(g, W):
    """[W, n_src] slots of every row inside every one of W windows of ceil(n_dst / W) ids, from the edge list."""
    w, _ = record_offsets(g, W)
    cnt = np.zeros((W, g.n_src), dtype=np.int64)
    np.add.at(cnt, (w, g.src.numpy()), 1)
    return cnt


def greedy_cut(slots, cap):
    """First vrow index of every part of one task, from its vrows' slot counts (csrc/tile_layout.h: do_task)."""
    starts, i = [], 0
    while i < len(slots):
        acc, j = 0, i
        while j < len(slots) and acc + slots[j] <= cap:
            acc += slots[j]
            j += 1
        if acc == 0:
            break
        assert j > i
        starts.append(i)
        i = j
    return starts


# ---- ragged last tile --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged_case(n_rows):
    return graph_case(dense_rows_graph(n_rows, 4 * WIN_IDS, 24, seed=100 + n_rows), 200 + n_rows)


@pytest.mark.parametrize("shape", ["R+5", "R+G+3", "7"])
@pytest.mark.parametrize("rows", [128, 192, 256, 384])
def test_ragged_last_tile(dev, rows, shape):
    """V vrows at R per tile: V = R + 5 (a last tile shorter than the G lane groups: most groups stage nothing), V = R + G + 3
    (a last tile of G + 3: the groups' second vrows are a mix of present and absent) and V = 7 (a single short tile).  24
    edges per row over 512 columns = 4 windows, rows left whole (vrow_t = 64).  Proof: the window structure's V."""
    G = GROUPS[rows]
    V = {"R+5": rows + 5, "R+G+3": rows + G + 3, "7": 7}[shape]
    c = ragged_case(V)

    def prove(info, plan):
        assert sweeps_of(plan) == [(4, WIN_IDS, 64, V)]
        last = V - (-(-V // rows) - 1) * rows
        assert last % G != 0 and (last < G or shape == "R+G+3")
    check_stage(c, dev, prove, sddmm_tile_rows=rows, vrow_t=64)


# ---- mixed predicate inside one lane group's loads ---------------------------------------------------------------------------
def mixed_graph(n_rows, rows_per_tile, seed):
    """30 edges per row over 4 windows of 128 ids: rows r % 3 == 0 draw from windows 0 and 2 only, the rows of the second
    tile from windows 0, 1 and 3 only, every other row from all four."""
    gen = torch.Generator().manual_seed(seed)
    r = torch.arange(n_rows)
    allowed = torch.ones(n_rows, 4, dtype=torch.bool)
    allowed[r % 3 == 0, 1] = False
    allowed[r % 3 == 0, 3] = False
    allowed[(r >= rows_per_tile) & (r < 2 * rows_per_tile), 2] = False
    win = torch.multinomial(allowed.float(), 30, replacement=True, generator=gen)
    dst = win * WIN_IDS + torch.randint(0, WIN_IDS, (n_rows, 30), generator=gen)
    return graphs.graph_from_coo(r.repeat_interleave(30), dst.reshape(-1), n_rows, 4 * WIN_IDS, 32)


@pytest.mark.parametrize("rows", [192, 256])
def test_mixed_predicate_inside_a_groups_loads(dev, rows):
    """Every third vrow has no slot in the odd windows and the whole second tile none in window 2, so a lane group's R / G A-row
    requests of one task are a mix of issued and skipped ones (its vrows g, g + G, ... differ modulo 3: G = 32 or 64), and one
    task requests none.  Rows left whole.  Proof: the per-(window, row) slot counts from the edge list, and V = rows."""
    n = 2 * rows + 40
    g = mixed_graph(n, rows, seed=rows)
    cnt = window_counts(g, 4)
    third = np.arange(n) % 3 == 0
    second = (np.arange(n) >= rows) & (np.arange(n) < 2 * rows)
    assert (cnt[1][third] == 0).all() and (cnt[3][third] == 0).all() and cnt[2][second].sum() == 0 and (cnt.sum(0) == 30).all()
    G = GROUPS[rows]
    for w in (1, 3):                                   # every lane group of the first tile: some of its vrows with, some without
        has = (cnt[w, :rows] > 0).reshape(rows // G, G)
        assert has.any(0).all() and not has.all(0).any(), w
    c = graph_case(g, 300 + rows)

    def prove(info, plan):
        assert sweeps_of(plan) == [(4, WIN_IDS, 64, n)]
    check_stage(c, dev, prove, sddmm_tile_rows=rows, vrow_t=64)


# ---- later parts: the write-out's entries by vrow index -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def parts_case(name):
    if name == "whole_rows":
        return graph_case(dense_rows_graph(400, 1024, 300, seed=32), 401)
    return graph_case(dense_rows_graph(400, 1024, 800, seed=34, lo_share=0.95), 402)


def piece_counts(g, piece, W):
    """[W, V] slots per window of every row piece when each row's slots, ascending by column, are cut into pieces of `piece`
    slots (the window structure's vrows), and the number of pieces of every row."""
    src, dst = g.src.numpy(), g.dst.numpy()
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    deg = np.bincount(src, minlength=g.n_src)
    first = np.concatenate([[0], np.cumsum(deg)])[:-1]
    pieces = -(-deg // piece)
    vfirst = np.concatenate([[0], np.cumsum(pieces)])
    vrow = vfirst[src] + (np.arange(len(src)) - first[src]) // piece
    cnt = np.zeros((W, int(vfirst[-1])), dtype=np.int64)
    np.add.at(cnt, (dst // (-(-g.n_dst // W)), vrow), 1)
    return cnt, pieces


@pytest.mark.parametrize("touch", [0, 1])
@pytest.mark.parametrize("name", ["whole_rows", "inside_a_row"])
def test_later_parts_begin_between_the_groups_strides(dev, name, touch):
    """192 rows per tile, two windows of 512 ids.  whole_rows: 400 rows of 300 slots left whole, a part holds some 50 of
    them.  inside_a_row: rows of 800 slots cut into 13 pieces of 64 (95 % of the columns in window 0), a part holds some
    130 pieces and begins inside a row.  A later part begins at a vrow index that is no multiple of G = 32, so its
    write-out takes the entries of other vrows than the group staged, in another order than they were staged.  With and without
    the touches of the next task's lines.  Proof: the greedy cut restated from the edge list at the library's cap has a
    later part at such an index (and, inside_a_row, at a vrow that is not a row's first piece), its largest part count equals
    sddmm_tile_max_parts >= 2, and the window structure is the one the restatement assumes."""
    rows, G, cap = 192, GROUPS[192], cap_of(192)
    c = parts_case(name)
    piece = 1024 if name == "whole_rows" else 64
    cnt, pieces = piece_counts(c.g, piece, 2)
    V = cnt.shape[1]
    per_row = 1 if name == "whole_rows" else 13
    assert (pieces == per_row).all() and V == per_row * c.g.n_src
    cuts = {(w, t): greedy_cut(cnt[w, t * rows:(t + 1) * rows], cap) for w in range(2) for t in range(-(-V // rows))}
    later = [(t * rows + s, s) for (w, t), ss in cuts.items() for s in ss[1:]]
    assert any(s % G != 0 for _, s in later), later
    if name == "inside_a_row":
        assert any(v % 13 != 0 and s % G != 0 for v, s in later), later
    else:
        assert (task_parts_uncut(c.g, 2, rows, cap) == np.array([[len(cuts[(w, t)]) for t in range(-(-V // rows))] for w in range(2)])).all()

    def prove(info, plan):
        assert sweeps_of(plan) == [(2, 512, piece, V)]
        assert info.sddmm_tile_max_parts == max(len(ss) for ss in cuts.values()) >= 2, (info.sddmm_tile_max_parts, cuts)
    check_stage(c, dev, prove, sddmm_tile_rows=rows, sweep_w=2, vrow_t=piece, sddmm_tile_touch=touch)


# ---- the result buffer's size -----------------------------------------------------------------------------
def boundary_graph(slots_in_window_0, seed):
    """192 + 40 rows over two windows of 512 ids; the first 192 rows -- one tile -- hold exactly slots_in_window_0 slots in
    window 0, spread evenly, and five each in window 1; the last 40 rows three in each window."""
    gen = torch.Generator().manual_seed(seed)
    n0 = torch.full((192,), slots_in_window_0 // 192)
    n0[:slots_in_window_0 % 192] += 1
    src = [torch.arange(192).repeat_interleave(n0), torch.arange(192).repeat_interleave(5), torch.arange(192, 232).repeat_interleave(6)]
    dst = [torch.randint(0, 512, (int(n0.sum()),), generator=gen), torch.randint(512, 1024, (192 * 5,), generator=gen),
           torch.cat([torch.randint(0, 512, (40, 3), generator=gen), torch.randint(512, 1024, (40, 3), generator=gen)], 1).reshape(-1)]
    return graphs.graph_from_coo(torch.cat(src), torch.cat(dst), 232, 1024, 32)


@pytest.mark.parametrize("over", [0, 1])
def test_a_task_of_exactly_the_buffer_and_of_one_slot_more(dev, over):
    """The buffer's size is the library's figure (choose_tile), not a literal of this file.  A task of exactly
    graphop_sddmm_tile_cap(192) slots is one part, one of a slot more is two (the second holds the tile's last row alone).
    Rows left whole.  Proof: the task's slot count from the edge list, the restated cut at the library's cap, and
    sddmm_tile_max_parts == 1 / 2 (no other task comes near the cap)."""
    cap = cap_of(192)
    g = boundary_graph(cap + over, seed=50 + over)
    cnt = window_counts(g, 2)
    assert cnt[0, :192].sum() == cap + over and cnt[1, :192].sum() == 192 * 5 and cnt[:, 192:].sum() == 240 and cnt.max() <= 1024
    parts = task_parts_uncut(g, 2, 192, cap)
    assert parts.tolist() == [[1 + over, 1], [1, 1]], parts
    c = graph_case(g, 500 + over)

    def prove(info, plan):
        assert sweeps_of(plan) == [(2, 512, 1024, 232)]
        assert info.sddmm_tile_max_parts == 1 + over
    check_stage(c, dev, prove, sddmm_tile_rows=192, sweep_w=2, vrow_t=1024)


# ---- a 1024-thread geometry, records of four slots ---------------------------------------------------------------------------
def test_hub_column_in_every_row_at_384_rows_per_tile(dev):
    """One workgroup of 1024 threads per CU, six vrows per lane group.  Column 233 sits in every one of 700 rows (20 k uniform
    edges besides): every tile holds at least 316 of its slots, which the plan packs into records of four -- their four
    results per lane go through the buffer and the write-out.  Proof: the column's count per tile from the edge list; rows
    left whole, so the window structure's V is the row count."""
    g0 = random_graph(700, 700, 20000, seed=6, chunk_size=32)
    g = graphs.graph_from_coo(torch.cat([g0.src, torch.arange(700)]), torch.cat([g0.dst, torch.full((700,), 233)]), 700, 700, 32)
    hub = np.bincount(g.src.numpy()[g.dst.numpy() == 233] // 384, minlength=2)
    assert hub.tolist()[0] >= 384 and hub.tolist()[1] >= 316
    assert int(torch.bincount(g.src).max()) <= 128
    c = graph_case(g, 600)

    def prove(info, plan):
        (W, win_cols, T, V), = sweeps_of(plan)
        assert (T, V) == (128, 700) and win_cols <= WIN_IDS and 233 // win_cols < W
    check_stage(c, dev, prove, sddmm_tile_rows=384, vrow_t=128)
