"""CPU tier of the bfloat16 fused attention step (kernels_attn_bf16.h): the ABI number stays, the plain
op's four entry points take dtype 2 and answer the stated workspace sums, shapes outside the set are not fused, empty
problems touch nothing, and the gfx950 code object keeps every k_attn_bf16_* kernel out of scratch.  Plans are the
host-side stand-ins of test_attention_heads_host.py, with the facts the bf16 form reads."""
import ctypes
import os
import re
import sys

import pytest

from test_attention_heads_host import _is_fused, _plan_struct, _query, _up

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD = [(1, 64), (1, 128), (2, 32), (2, 64), (4, 16), (4, 32), (4, 64), (8, 8), (8, 16), (8, 32), (8, 64)]
BF16, QUERY = 2, "attention_workspace_bytes"


def _plan(n_chunks, n_edges, max_row, max_index, row_owned=1, indices=True):
    plan = _plan_struct()()
    plan.info.n_chunks, plan.info.n_edges, plan.info.max_row, plan.info.max_index = n_chunks, n_edges, max_row, max_index
    plan.info.rows_sorted = plan.info.indptr_monotone = plan.info.row_owned = row_owned
    plan.indices = 256 if indices else None
    return plan


@pytest.fixture
def lib():
    from custom_op_benchmark_amd import _lib
    _lib.tune_reset()
    yield _lib.lib()
    _lib.tune_reset()


def test_abi_number_and_the_attention_only_dtype(lib):
    import torch
    from custom_op_benchmark_amd import _lib
    assert _lib.ABI_VERSION == 8 and lib.graphop_abi_version() == 8 and _lib.BF16 == BF16
    x = torch.zeros(2, dtype=torch.bfloat16)
    assert _lib.attn_dtype_code("attention_forward", x) == _lib.attn_dtype_code("attention_backward", x) == BF16
    for fn in ("attention_dropout_forward", "attention_bias_backward"):
        with pytest.raises(RuntimeError, match="float32 / float64 only"):
            _lib.attn_dtype_code(fn, x)
    assert _lib.attn_stats_dtype(x) == torch.float32 and _lib.attn_stats_dtype(x.double()) == torch.float64


def test_workspace_queries_answer_the_stated_sums(lib):
    """E = 1000 edges, 100 row-major and 107 column-major chunks, n_q = 50, n_k = 40: one chunk per lane group (so few
    chunks are fewer than the groups wanted on any device), two record slots per group."""
    E, C, n_q, n_k = 1000, 100, 50, 40
    pr, pc = _plan(C, E, n_q - 1, n_k - 1), _plan(C + 7, E, n_k - 1, n_q - 1)
    for h, d in ((4, 16), (8, 64)):
        F, np_r, np_c = h * d, 2 * C, 2 * (C + 7)
        # forward records: row word | (m, l) per head | o row, all 4-byte words
        fwd = _up(4 * np_r) + _up(4 * np_r * 2 * h) + _up(4 * np_r * F)
        # backward: packed (K | V) and (Q | dO) of 2 F bf16 per node, stats4 per (query row, head), then the records of
        # the pass that is running -- row words and accumulator rows for the larger of the two passes (np_r x F floats
        # against np_c x 2 F)
        bwd = _up(2 * n_k * 2 * F) + _up(2 * n_q * 2 * F) + _up(16 * n_q * h) + _up(4 * np_c) + _up(4 * 2 * np_c * F)
        assert _query(lib, QUERY, 0, E, n_q, n_k, h, d, pr, pc, dtype=BF16) == fwd, (h, d)
        assert _query(lib, QUERY, 0, E, n_q, n_k, h, d, pr, None, dtype=BF16) == fwd, (h, d)
        assert _query(lib, QUERY, 1, E, n_q, n_k, h, d, pr, pc, dtype=BF16) == bwd, (h, d)
    # the other queries keep answering dtype 2 as before
    out = ctypes.c_int64(-1)
    n = ctypes.c_void_p(0)
    assert lib.graphop_attention_dropout_workspace_bytes(BF16, 0, E, n_q, n_k, 4, 16, ctypes.byref(pr), n, n,
                                                         ctypes.byref(out)) == 1
    assert b"attention_dropout_workspace_bytes: bad dtype" in lib.graphop_last_error()


def test_is_fused_inside_and_outside_the_set(lib):
    from custom_op_benchmark_amd import _lib
    E, C, n = 1000, 100, 50
    pr, pc = _plan(C, E, n - 1, n - 1), _plan(C, E, n - 1, n - 1)
    for knob in (None, "attn_heads", "attn_rows", "force_generic"):          # no knob steers the one bf16 form
        if knob:
            _lib.tune(knob, 1 if knob == "force_generic" else 0)
        for h, d in HD:
            assert _is_fused(lib, E, n, n, h, d, pr, pc, dtype=BF16) == 1, (knob, h, d)
        _lib.tune_reset()
    for h, d in ((3, 8), (2, 16), (1, 32), (1, 256), (16, 16), (4, 8), (8, 128), (6, 16)):
        assert _is_fused(lib, E, n, n, h, d, pr, pc, dtype=BF16) == 0, (h, d)
        assert _query(lib, QUERY, 1, E, n, n, h, d, pr, pc, dtype=BF16) == 0
    # an unsorted chunk list, id ranges outside the tables, a plan without neighbour ids, an empty graph
    for bad_r, bad_c in ((_plan(C, E, n - 1, n - 1, row_owned=0), pc), (pr, _plan(C, E, n - 1, n - 1, row_owned=0)),
                         (_plan(C, E, n, n - 1), pc), (pr, _plan(C, E, n - 1, n)),
                         (_plan(C, E, n - 1, n - 1, indices=False), pc)):
        assert _is_fused(lib, E, n, n, 4, 16, bad_r, bad_c, dtype=BF16) == 0
    assert _is_fused(lib, 0, 0, 0, 4, 16, _plan(0, 0, -1, -1), _plan(0, 0, -1, -1), dtype=BF16) == 0


def test_empty_problems_touch_nothing_and_unmet_conditions_are_named(lib):
    n = ctypes.c_void_p(0)
    for h, d in ((4, 16), (8, 64)):
        assert lib.graphop_attention_forward(BF16, *([n] * 7), n, n, 0, 0, 0, 7, h, d, n, 0, n, n) == 0
        assert lib.graphop_attention_backward(BF16, *([n] * 11), *([n] * 6), 0, 0, 0, 0, 0, h, d, n, 0, n, n, n) == 0
    # with edges and no plan the op refuses, naming the condition, before it reads an array
    some = ctypes.c_void_p(4096)
    assert lib.graphop_attention_forward(BF16, *([some] * 7), some, some, 4, 10, 5, 5, 4, 16, n, 0, n, n) == 1
    assert b"attention_forward: bfloat16 unsupported: plan is NULL" in lib.graphop_last_error()
    assert lib.graphop_attention_forward(BF16, *([some] * 7), some, some, 4, 10, 5, 5, 3, 8, n, 0, n, n) == 1
    assert b"(h, d) = (3, 8) is not in the bfloat16 set" in lib.graphop_last_error()
    assert lib.graphop_attention_bias_forward(BF16, *([some] * 8), some, some, 4, 10, 5, 5, 4, 16, n, 0, n, n, 0.0, 0, 0,
                                              0) == 1
    assert b"attention_bias_forward: bad dtype" in lib.graphop_last_error()


def test_bf16_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    fam = {}
    for name, r in kernel_resources().items():
        m = re.search(r"graphop::(k_attn_bf16_\w+)<(.*)>\(", name)
        if m:
            assert not r["spill_vgpr"] and not r["scratch"] and r["vgpr"] <= 256, (name, r)
            assert not re.search(r"_f32<", name), name          # clear of the patterns that pin the fp32 kernels
            fam.setdefault(m.group(1), set()).add(m.group(2))
    hd = ["%d, %d" % x for x in HD]
    both = {a + ", " + b for a in hd for b in ("false", "true")}
    assert fam == {"k_attn_bf16_fwd_rows": set(hd), "k_attn_bf16_fwd_merge": set(hd), "k_attn_bf16_pack": both,
                   "k_attn_bf16_bwd_rows": both, "k_attn_bf16_bwd_merge": both}
