"""CPU tier of the several-head forms of the fused dot-product attention ops (kernels_attn_heads.h): the
entry points and the knob exist in both bindings, the ABI number stays, the workspace queries answer the stated sums,
empty problems touch nothing, shapes outside the set are not fused, and the gfx950 code object keeps every
k_attn_heads_* kernel out of scratch.

The decision needs plans, and a plan needs a device.  The queries only read a plan's facts (graphop_plan_info_t) and
whether it carries neighbour ids, so the tests hand them a host-side stand-in: a zeroed graphop_plan (csrc/common.h)
with the facts filled in."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD = [(2, 32), (2, 64), (4, 16), (4, 32), (4, 64), (8, 8), (8, 16), (8, 32)]
NAMES = ("attention_forward", "attention_backward", "attention_dropout_forward", "attention_dropout_backward",
         "attention_bias_forward", "attention_bias_backward")
QUERIES = ("attention_workspace_bytes", "attention_dropout_workspace_bytes", "attention_bias_workspace_bytes")


def _plan_struct():
    from custom_op_benchmark_amd import _lib
    p = ctypes.c_void_p

    class Plan(ctypes.Structure):          # struct graphop_plan of csrc/common.h
        _fields_ = [("info", _lib.PlanInfo), ("sorted_in_rows", ctypes.c_int), ("sweeps", p), ("sweep_mu", p), ("walks", p),
                    ("row", p), ("indptr", p), ("eid", p), ("indices", p), ("seg_chunk", p), ("seg_eptr", p), ("idx32", p),
                    ("eid32", p), ("long_segs", p), ("n_long", ctypes.c_int64), ("blk_seg", p), ("seg_e0", p),
                    ("seg_row", p), ("device", ctypes.c_int), ("mirrors_pinned", ctypes.c_int)]
    return Plan


def _plan(n_chunks, n_edges, max_row, max_index, rows_sorted=1, indices=True):
    """a stand-in plan: the facts the several-head decision reads, no device array behind it"""
    plan = _plan_struct()()
    plan.info.n_chunks, plan.info.n_edges, plan.info.max_row, plan.info.max_index = n_chunks, n_edges, max_row, max_index
    plan.info.rows_sorted = rows_sorted
    plan.info.eid_identity = 1
    plan.indices = 256 if indices else None
    return plan


def _up(v):
    return (v + 255) // 256 * 256


def _query(l, which, backward, E, n_q, n_k, h, d, plan_r, plan_c, dtype=0, with_db=None):
    out = ctypes.c_int64(-1)
    n = ctypes.c_void_p(0)
    extra = () if with_db is None else (with_db,)
    assert getattr(l, "graphop_" + which)(dtype, backward, E, n_q, n_k, h, d, ctypes.byref(plan_r) if plan_r else n,
                                          ctypes.byref(plan_c) if plan_c else n, n, *extra, ctypes.byref(out)) == 0, \
        l.graphop_last_error()
    return out.value


def _is_fused(l, E, n_q, n_k, h, d, plan_r, plan_c, dtype=0):
    out = ctypes.c_int(-1)
    assert l.graphop_attention_backward_is_fused(dtype, E, n_q, n_k, h, d, ctypes.byref(plan_r), ctypes.byref(plan_c),
                                                 ctypes.c_void_p(0), ctypes.byref(out)) == 0, l.graphop_last_error()
    return out.value


@pytest.fixture
def lib():
    from custom_op_benchmark_amd import _lib
    _lib.tune_reset()
    yield _lib.lib()
    _lib.tune_reset()


def test_symbols_and_knob_in_both_bindings(lib):
    from custom_op_benchmark_amd import _ext, _lib, functions, graphop as ops
    l = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES + QUERIES + ("attention_backward_is_fused",):
        assert hasattr(l, "graphop_" + n) and "graphop_" + n in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 8 and lib.graphop_abi_version() == 8          # additive: the ABI number stays
    ext = _ext.load()
    assert ext is not None, "graphop_cpp.so not built (run __graft_entry__.build())"
    for n in NAMES:
        assert callable(getattr(ext, n)) and callable(getattr(ops, n))
    # nothing new under torch.ops.graphop: the several-head form has no entry point of its own
    assert not [n for n in list(ops._SCHEMAS) + list(ops.EXTRA_OPS) + list(ops.__all__) if "attention_heads" in n]
    # the knob: -1 by default, settable and enumerable through either binding's library
    assert _lib.tune_get("attn_heads") == -1 and "attn_heads" in _lib.tune_snapshot()
    for v in (0, 1, -1):
        _lib.tune("attn_heads", v)
        assert _lib.tune_get("attn_heads") == v
    _lib.tune("attn_heads", 1); _lib.tune_reset()
    assert _lib.tune_get("attn_heads") == -1
    assert callable(functions._heads_per_call) and functions._head_group(8, 32) == 2 and functions._head_group(8, 64) == 1


def test_workspace_queries_answer_the_stated_sums(lib):
    """E = 1000 edges in 100 chunks, n_q = 50, n_k = 40, 4 x 16 (F = 64): one chunk per lane group (100 chunks are fewer
    than the groups wanted on any device), so 100 groups and 200 piece records."""
    from custom_op_benchmark_amd import _lib
    E, C, n_q, n_k, h, d = 1000, 100, 50, 40, 4, 16
    F, groups = h * d, 100
    pr, pc = _plan(C, E, n_q - 1, n_k - 1), _plan(C + 7, E, n_k - 1, n_q - 1, rows_sorted=0)
    _lib.tune("attn_heads", 1)
    # forward: piece records of 2 * groups * (1 + 2 h + F) words (row word | (m, l) per head | o), Mtmp and Ltmp of n_q * h
    fwd = _up(4 * 2 * groups) + _up(4 * 2 * groups * 2 * h) + _up(4 * 2 * groups * F) + 2 * _up(4 * n_q * h)
    assert fwd == 1024 + 6400 + 51200 + 2 * 1024
    # backward: the packed (K | V) and (Q | dO) tables of 2 F floats per node, stats4 of (n_q + n_k) * h float4
    bwd = _up(4 * n_k * 2 * F) + _up(4 * n_q * 2 * F) + _up(16 * (n_q + n_k) * h)
    assert bwd == 20480 + 25600 + 5888
    for which, extras in ((QUERIES[0], (None,)), (QUERIES[1], (None,)), (QUERIES[2], (0, 1))):
        for with_db in extras:          # db is the caller's: the workspace is the same with and without it
            assert _query(lib, which, 0, E, n_q, n_k, h, d, pr, pc, with_db=with_db) == fwd, (which, with_db)
            assert _query(lib, which, 1, E, n_q, n_k, h, d, pr, pc, with_db=with_db) == bwd, (which, with_db)
    assert _is_fused(lib, E, n_q, n_k, h, d, pr, pc) == 1
    # a forward whose rows are not sorted composes (s and a: two (E, h) arrays + the softmax scratch); its backward is fused
    assert _query(lib, QUERIES[2], 0, E, n_k, n_q, h, d, pc, pr, with_db=0) >= 2 * _up(4 * E * h)
    # knobs: either 0 gives the composed answers of the calls without plans
    composed = [_query(lib, QUERIES[2], bw, E, n_q, n_k, h, d, None, None, with_db=1) for bw in (0, 1)]
    for knob in ("attn_heads", "attn_rows", "attn_fused"):
        _lib.tune_reset(); _lib.tune("attn_heads", 1); _lib.tune(knob, 0)
        assert [_query(lib, QUERIES[2], bw, E, n_q, n_k, h, d, pr, pc, with_db=1) for bw in (0, 1)] == composed, knob
        assert _is_fused(lib, E, n_q, n_k, h, d, pr, pc) == 0
    # auto: with a tenth of the edges the E-sized streams avoided ((144 + 36 h) E = 28 800 B) do not pay for packing the
    # tables (32 F (n_q + n_k) = 184 320 B): composed; the knob 1 still reaches the form
    _lib.tune_reset()
    assert (144 + 36 * h) * 100 <= 32 * F * (n_q + n_k)
    small_r, small_c = _plan(C, 100, n_q - 1, n_k - 1), _plan(C, 100, n_k - 1, n_q - 1)
    assert _is_fused(lib, 100, n_q, n_k, h, d, small_r, small_c) == 0
    _lib.tune("attn_heads", 1)
    assert _is_fused(lib, 100, n_q, n_k, h, d, small_r, small_c) == 1


def test_shapes_outside_the_set_are_not_fused(lib):
    from custom_op_benchmark_amd import _lib
    E, C, n = 1000, 100, 50
    pr, pc = _plan(C, E, n - 1, n - 1), _plan(C, E, n - 1, n - 1)
    _lib.tune("attn_heads", 1)
    for h, d in HD:
        assert _is_fused(lib, E, n, n, h, d, pr, pc) == 1, (h, d)
        assert _is_fused(lib, E, n, n, h, d, pr, pc, dtype=1) == 0, (h, d)          # fp64
    for h, d in ((3, 8), (2, 16), (2, 8), (8, 64), (16, 16), (4, 8), (8, 4), (2, 128), (6, 16), (4, 24)):
        assert _is_fused(lib, E, n, n, h, d, pr, pc) == 0, (h, d)
        assert _query(lib, QUERIES[0], 1, E, n, n, h, d, pr, pc) >= 4 * _up(4 * E * h)          # the composed backward
    # id ranges outside the tables, a plan without neighbour ids: not this form
    assert _is_fused(lib, E, n, n, 4, 16, _plan(C, E, n, n - 1), pc) == 0
    assert _is_fused(lib, E, n, n, 4, 16, pr, _plan(C, E, n - 1, n)) == 0
    assert _is_fused(lib, E, n, n, 4, 16, _plan(C, E, n - 1, n - 1, indices=False), pc) == 0


def test_empty_problems_touch_nothing(lib):
    from custom_op_benchmark_amd import _lib
    _lib.tune("attn_heads", 1)
    n = ctypes.c_void_p(0)

    def fwd(C, E, n_q, n_k, h, d, p=0.0, head0=0):
        return lib.graphop_attention_bias_forward(0, *([n] * 7), n, n, n, C, E, n_q, n_k, h, d, n, 0, n, n, p, 0, 0, head0)

    def bwd(C, C2, E, n_q, n_k, h, d, p=0.0, head0=0):
        return lib.graphop_attention_bias_backward(0, *([n] * 11), n, *([n] * 7), C, C2, E, n_q, n_k, h, d, n, 0, n, n, n,
                                                   p, 0, 0, head0)

    for h, d in ((4, 16), (8, 32)):
        assert fwd(0, 0, 0, 0, h, d) == 0 and fwd(0, 0, 0, 7, h, d, 0.6, 4) == 0, lib.graphop_last_error()
        assert bwd(0, 0, 0, 0, 0, h, d) == 0 and bwd(0, 0, 0, 0, 0, h, d, 0.6, 2) == 0, lib.graphop_last_error()
        assert lib.graphop_attention_forward(0, *([n] * 7), n, n, 0, 0, 0, 0, h, d, n, 0, n, n) == 0
        assert lib.graphop_attention_dropout_forward(0, *([n] * 7), n, n, 0, 0, 0, 0, h, d, n, 0, n, n, 0.5, 1, 0, 0) == 0
    # with plans of an empty graph the queries answer, and the decision is "not fused"
    empty = _plan(0, 0, -1, -1)
    assert _query(lib, QUERIES[2], 0, 0, 0, 0, 4, 16, empty, empty, with_db=1) >= 0
    assert _query(lib, QUERIES[2], 1, 0, 0, 0, 4, 16, empty, empty, with_db=1) >= 0
    assert _is_fused(lib, 0, 0, 0, 4, 16, empty, empty) == 0


def test_heads_kernels_do_not_spill():
    """Every k_attn_heads_* instantiation: no scratch, no spilled VGPR; forward, backward, pack and merge kernels exist
    for every (H, D) of the set and every combination of their options."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources()
    heads = {n: r for n, r in res.items() if "graphop::k_attn_heads_" in n}
    fam = {}
    for n, r in heads.items():
        m = re.search(r"graphop::(k_attn_heads_\w+?)(?:<(.*)>)?\(", n)
        assert m, n
        fam.setdefault(m.group(1), {})[m.group(2)] = r
        assert not r["spill_vgpr"] and not r["scratch"], (n, r)
    assert set(fam) == {"k_attn_heads_fwd_rows_f32", "k_attn_heads_bwd_rows_f32", "k_attn_heads_pack", "k_attn_heads_piece_max",
                        "k_attn_heads_piece_add", "k_attn_heads_piece_fin"}, sorted(fam)
    hd = ["%d, %d" % x for x in HD]
    tf = ("false", "true")
    assert set(fam["k_attn_heads_fwd_rows_f32"]) == {", ".join((a, dr, bi)) for a in hd for dr in tf for bi in tf}
    assert set(fam["k_attn_heads_bwd_rows_f32"]) == {", ".join((a, c, o, dr, bi)) for a in hd for c in tf for o in tf
                                                     for dr in tf for bi in tf}
    assert set(fam["k_attn_heads_pack"]) == {", ".join((a, s)) for a in hd for s in tf}
    assert set(fam["k_attn_heads_piece_add"]) == set(hd) == set(fam["k_attn_heads_piece_fin"])
    # the names stay clear of the patterns that pin the one-head kernels (tests/test_attention_dropout_host.py, _bias_host.py)
    assert not [n for n in heads if re.search(r"k_attn_(bwd_rows|bwd_wown|fwd_walk|bias_\w+)_f32<", n)]
    spilled = {n: r["spill_sgpr"] for n, r in heads.items() if r["spill_sgpr"]}
    print("k_attn_heads_* kernels that spill SGPRs (DESIGN.md 4.5l records them):", spilled)
    worst = max(r["vgpr"] for r in heads.values())
    assert worst <= 256, worst          # two workgroups of 256 threads per CU at the least
