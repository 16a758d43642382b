"""CPU tier of the fused dot-product attention step with an edge-type score bias (graphop_attention_tbias_*, DESIGN.md
4.5p): the library and the bindings expose the ops and validate their arguments before anything touches a device, the
gfx950 code object holds exactly the k_attn_tbias_* instantiations the op launches and keeps every one out of scratch,
and the inputs the GPU tier uses are ones on which torch's own fp32 arithmetic stays within half of that tier's bounds."""
import ctypes
import os
import re
import sys

import pytest
import torch

import attention_bias_reference as AB
import attention_tbias_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("attention_tbias_forward", "attention_tbias_backward")
CLAMP = "never touches memory outside B / dB"


def test_reference_is_the_bias_reference_on_gathered_values():
    """the statement itself: o, dQ, dK, dV are attention_bias_reference's on b = B[etype], dB sums db per type, a type no
    edge carries gets exactly 0, parallel edges may differ in type, out-of-range types read as the last one, and the
    input sets hold what the GPU tier relies on"""
    g, inp, n_types = T.input_set("pair_4_16")
    Q, K, V, B, etype, dO = inp
    want = T.reference_step(g.src, g.dst, g.n_src, *inp, *T.DROP)
    bias = AB.reference_step(g.src, g.dst, g.n_src, Q, K, V, B[etype.long()], dO, *T.DROP)
    for k in T.PLAIN:
        torch.testing.assert_close(want[k], bias[k], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(want["db"], bias["db"], rtol=1e-12, atol=1e-12)
    has = torch.bincount(g.src, minlength=g.n_src) > 0
    torch.testing.assert_close(want["stats"][has], bias["stats"][has], rtol=1e-12, atol=1e-12)
    assert (want["stats"][~has][..., 0] == -1e9).all() and not want["stats"][~has][..., 1].any()
    assert want["dB"].shape == B.shape and want["db"].shape == (g.n_edges, 4)
    count = torch.bincount(etype.long(), minlength=n_types)
    assert count[-1] == 0 and not want["dB"][-1].any() and want["dB"][:-1].abs().min() > 0
    hub = T.hub_row(g)
    assert count[-2] >= 75 and (g.src[etype == n_types - 2] == hub).all()
    for t in range(n_types):
        torch.testing.assert_close(want["dB"][t], want["db"][etype == t].sum(0), rtol=1e-12, atol=1e-12)
    pair = g.src * g.n_dst + g.dst
    order = torch.argsort(pair, stable=True)
    twin = order[:-1][(pair[order][1:] == pair[order][:-1]) & (etype[order][1:] != etype[order][:-1])]
    assert twin.numel() > 0          # parallel edges of different types
    bad = torch.tensor([-1, n_types, 2 ** 31 - 1, -2 ** 31, 0, n_types - 1], dtype=torch.int32)
    assert T.clamped(bad, n_types).tolist() == [n_types - 1] * 4 + [0, n_types - 1]
    assert T.max_types(8) == 512 and T.max_types(1) == 4096 and T.max_types(4) == 1024
    assert {"types_1", "types_512", "types_513"} <= set(T.INPUT_SETS)
    deg = torch.bincount(g.src, minlength=g.n_src)
    assert deg.max() >= 150 and (g.ptr_r[1:] - g.ptr_r[:-1]).max() <= 8 and (deg == 0).any()


def test_symbols_resolve_in_the_library_and_the_extension():
    from custom_op_benchmark_amd import _ext, _lib, functions, graphop as ops
    l = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES + ("attention_tbias_workspace_bytes",):
        assert hasattr(l, "graphop_" + n) and "graphop_" + n in _lib.EXPORTED_SYMBOLS
        assert "graphop_" + n in _lib._SIGNATURES
        assert _lib._SIGNATURES["graphop_" + n] == _lib._SIGNATURES["graphop_" + n.replace("tbias", "etype")]
    header = open(os.path.join(ROOT, "include", "graphop_hip.h")).read()
    for n in NAMES + ("attention_tbias_workspace_bytes",):
        assert re.search(r"GRAPHOP_API int graphop_%s\(" % n, header), n
    assert CLAMP in header          # the clamp is stated where the ABI is
    assert _lib.ABI_VERSION == 8 and _lib.lib().graphop_abi_version() == 8        # additive: the ABI number stays
    ext = _ext.load()
    assert ext is not None, "graphop_cpp.so not built (run __graft_entry__.build())"
    for n in NAMES:
        assert callable(getattr(ext, n)) and callable(getattr(ops, n))
        assert n in ops.EXTRA_OPS and n not in ops._SCHEMAS and not hasattr(torch.ops.graphop, n)
        assert "clamp" in getattr(ops, n).__doc__ and "memory outside B" in getattr(ops, n).__doc__
        doc = getattr(ext, n).__doc__.splitlines()[0]
        args = [a.split(":")[0] + (a[a.index(" = "):] if " = " in a else "") for a in doc[doc.index("(") + 1:doc.rindex(") -> ")].split(", ")]
        tail = ["p = 0.0", "seed = 0", "offset = 0", "head0 = 0"]
        if n.endswith("forward"):
            assert args[4:9] == ["Q", "K", "V", "B", "etype"] and args[9:] == tail, doc
        else:
            assert args[8:16] == ["Q", "K", "V", "B", "etype", "o", "stats", "dO"] and args[16:] == tail + ["need_dB = True"], doc
    assert issubclass(functions.FusedAttentionTypeBias, torch.autograd.Function)
    assert "clamp" in functions.FusedAttentionTypeBias.__doc__
    assert callable(functions.fused_attention_tbias_step) and callable(functions.attention_tbias_step)
    assert "FusedAttentionTypeBias" in functions.FusedAttentionBias.__doc__
    assert len(ops.__all__) == 8 and not set(NAMES) & set(ops.__all__)


def _fwd(l, dtype, C, E_, n_q, n_k, h, d, n_types, p=0.0, seed=0, offset=0, head0=0, B=None, etype=None, ws=None,
         ws_bytes=0):
    n = ctypes.c_void_p(0)
    return l.graphop_attention_tbias_forward(dtype, *([n] * 7), B or n, etype or n, n, n, C, E_, n_q, n_k, h, d, n_types,
                                             ws or n, ws_bytes, n, n, p, seed, offset, head0)


def _bwd(l, dtype, C, C2, E_, n_q, n_k, h, d, n_types, p=0.0, seed=0, offset=0, head0=0, B=None, etype=None, ws=None,
         ws_bytes=0):
    n = ctypes.c_void_p(0)
    return l.graphop_attention_tbias_backward(dtype, *([n] * 11), B or n, etype or n, *([n] * 7), C, C2, E_, n_q, n_k, h,
                                              d, n_types, ws or n, ws_bytes, n, n, n, p, seed, offset, head0)


def _ws(l, dtype, backward, E_, n_q, n_k, h, d, n_types):
    out = ctypes.c_int64(-1)
    n = ctypes.c_void_p(0)
    assert l.graphop_attention_tbias_workspace_bytes(dtype, backward, E_, n_q, n_k, h, d, n_types, n, n, n,
                                                     ctypes.byref(out)) == 0
    return out.value


def test_argument_validation_without_gpu():
    """error code 1 (GRAPHOP_ERR_ARG) and the text, through ctypes with dummy pointers: nothing touches a device"""
    from custom_op_benchmark_amd import _lib
    l = _lib.lib()
    some = ctypes.c_void_p(256)
    both = dict(B=some, etype=some)
    err = l.graphop_last_error
    assert _fwd(l, 7, 4, 10, 5, 5, 2, 8, 3, **both) == 1 and b"attention_tbias_forward: bad dtype" in err()
    assert _bwd(l, 2, 4, 4, 10, 5, 5, 2, 8, 3, **both) == 1 and b"attention_tbias_backward: bad dtype" in err()
    assert _bwd(l, 0, 0, -3, 0, 0, 0, 1, 8, 0) == 1 and b"negative" in err()
    for p in (1.0, -0.1, float("nan"), 1.5):
        assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, 3, p, **both) == 1 and b"p must be in [0, 1)" in err()
        assert _bwd(l, 0, 4, 4, 10, 5, 5, 2, 8, 3, p, **both) == 1 and b"p must be in [0, 1)" in err()
    assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, 3, 0.5, seed=2 ** 63, **both) == 1 and b"seed" in err()
    assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, 3, 0.5, head0=-1, **both) == 1 and b"head0 must be in [0, 2^32)" in err()
    assert _bwd(l, 0, 4, 4, 10, 5, 5, 2, 8, 3, 0.0, head0=2 ** 32, **both) == 1 and b"head0 must be in [0, 2^32)" in err()
    # the order: attn_check (dtype), then the dropout arguments, then n_types, then B, then etype, then the workspace
    assert _fwd(l, 7, 4, 10, 5, 5, 2, 8, 0, 1.5) == 1 and b"dtype" in err()
    assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, 0, 1.5) == 1 and b"p must be in [0, 1)" in err()
    assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, 0, 0.5, head0=-1) == 1 and b"head0" in err()
    for n_types in (0, -1):
        assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, n_types, 0.5) == 1 and b"attention_tbias_forward: n_types must be >= 1" in err()
        assert _bwd(l, 1, 4, 4, 10, 5, 5, 2, 8, n_types, **both) == 1 and b"attention_tbias_backward: n_types must be >= 1" in err()
    assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, 3, 0.5) == 1 and b"attention_tbias_forward: B is NULL" in err()
    assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, 3, 0.5, B=some) == 1 and b"attention_tbias_forward: etype is NULL" in err()
    assert _bwd(l, 1, 4, 4, 10, 5, 5, 2, 8, 3) == 1 and b"attention_tbias_backward: B is NULL" in err()
    assert _bwd(l, 1, 4, 4, 10, 5, 5, 2, 8, 3, B=some) == 1 and b"attention_tbias_backward: etype is NULL" in err()
    # short workspace: plan-less, the generic backward wants P (n_q, h, 4) in the op's dtype; the forward wants none.
    # B and etype NULL with a short workspace: the table is named, so it is checked before the workspace
    E_, n, h, d = 1000, 50, 2, 8
    for dtype, es in ((0, 4), (1, 8)):
        assert _ws(l, dtype, 0, E_, n, n, h, d, 3) == 0
        need = _ws(l, dtype, 1, E_, n, n, h, d, 3)
        assert need == (es * 4 * n * h + 255) // 256 * 256
        assert need == _ws(l, dtype, 1, E_, n, n, h, d, 5000)          # plan-less: no replicas, whatever n_types
        assert _bwd(l, dtype, 4, 4, E_, n, n, h, d, 3, 0.5, ws=some, ws_bytes=need - 1, **both) == 1
        assert b"attention_tbias_backward: workspace of %d bytes needed (graphop_attention_tbias_workspace_bytes)" % need in err()
        assert _bwd(l, dtype, 4, 4, E_, n, n, h, d, 3, 0.5, ws=None, ws_bytes=need, **both) == 1 and b"workspace" in err()
        assert _bwd(l, dtype, 4, 4, E_, n, n, h, d, 3, 0.5, ws=some, ws_bytes=need - 1) == 1 and b"B is NULL" in err()
    out = ctypes.c_int64(-1)
    n0 = ctypes.c_void_p(0)
    q = l.graphop_attention_tbias_workspace_bytes
    assert q(5, 1, 10, 5, 5, 2, 8, 3, n0, n0, n0, ctypes.byref(out)) == 1 and b"dtype" in err()
    assert q(0, 1, 10, 5, 5, 2, 8, -1, n0, n0, n0, ctypes.byref(out)) == 1 and b"negative" in err()
    assert q(0, 1, 10, 5, 5, 2, 8, 3, n0, n0, n0, None) == 1 and b"bytes_out" in err()


def test_empty_problems_without_gpu():
    """no-ops that never dereference anything, n_types == 0 allowed where there is no edge; their workspace is 0"""
    from custom_op_benchmark_amd import _lib
    l = _lib.lib()
    some = ctypes.c_void_p(256)
    assert _fwd(l, 0, 0, 0, 0, 0, 1, 8, 0, 0.6) == 0
    assert _fwd(l, 1, 0, 0, 0, 7, 4, 16, 0, 0.6, seed=2 ** 63 - 1, offset=2 ** 32 - 1, head0=4) == 0
    assert _fwd(l, 0, 4, 10, 0, 5, 2, 8, 3, B=some, etype=some) == 0          # no query rows
    assert _bwd(l, 0, 0, 0, 0, 0, 0, 1, 8, 0, 0.6) == 0
    assert _bwd(l, 1, 0, 0, 0, 0, 0, 3, 8, 2) == 0                 # dB NULL: nothing to fill
    assert _bwd(l, 0, 4, 4, 10, 5, 5, 2, 0, 3) == 0                # d == 0: B and etype may be NULL
    for backward in (0, 1):
        for dtype in (0, 1):
            for E_, n_q, n_k, h, d, nt in ((0, 0, 0, 1, 8, 0), (0, 5, 5, 2, 8, 0), (10, 0, 5, 2, 8, 3), (10, 5, 0, 2, 8, 3),
                                           (10, 5, 5, 2, 0, 3)):
                assert _ws(l, dtype, backward, E_, n_q, n_k, h, d, nt) == 0


def test_binding_refusals_without_gpu():
    """the dropout arguments first, then the tensors; the table is checked once per binding, in the same words"""
    from custom_op_benchmark_amd import graphop as ops
    i = torch.zeros(2, dtype=torch.int64)
    v = torch.zeros(2, 4, 8)
    st = torch.zeros(2, 4, 2)
    B = torch.zeros(3, 4)
    et = torch.zeros(2, dtype=torch.int32)
    for kw, msg in ((dict(p=0.5, offset=2 ** 32), "offset"), (dict(p=1.0), r"p must be in \[0, 1\)"),
                    (dict(p=float("nan")), r"p must be in \[0, 1\)"), (dict(p=0.5, seed=-1), "seed"),
                    (dict(p=0.5, head0=-1), "head0"), (dict(head0=2 ** 32), "head0")):
        for mod in (ops, ops.cpp_ext):
            with pytest.raises(RuntimeError, match=msg):
                mod.attention_tbias_forward(i, i, i, i, v, v, v, B, et, **kw)
            with pytest.raises(RuntimeError, match=msg):
                mod.attention_tbias_backward(i, i, i, i, i, i, i, i, v, v, v, B, et, v, st, v, **kw)
    for mod in (ops, ops.cpp_ext):
        with pytest.raises(RuntimeError, match="row must be a CUDA tensor"):
            mod.attention_tbias_forward(i, i, i, i, v, v, v, B, et)
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            mod.attention_tbias_backward(i, i, i, i, i, i, i, i, v, v, v, B, et, v, st, v)
    # the table against the graph and Q (graphop._attn_tbias_table; torch_ext.cpp's check_attn_tbias_table has the same
    # order and words, reached on the GPU tier): B's dtype, B's shape, an empty table, etype's dtype and shape,
    # contiguity and device
    shape = r"B must be \(n_types\) for 2-D Q / K / V, else \(n_types, h\)"
    for badB, bad_et, msg in (
            (torch.zeros(3, 4, dtype=torch.float64), et, "expected Q and B to have the same dtype"),
            (torch.zeros(3), et, shape), (torch.zeros(3, 8), et, shape), (torch.zeros(3, 4, 8), et, shape),
            (torch.zeros(3, 3), et, shape), (torch.zeros(0, 4), et, "B must hold at least one type"),
            (B, et.long(), "etype must be torch.int32"), (B, et.float(), "etype must be torch.int32"),
            (B, torch.zeros(3, dtype=torch.int32), r"etype must be \(n_edges\)"),
            (B, torch.zeros(2, 1, dtype=torch.int32), r"etype must be \(n_edges\)"),
            (torch.zeros(3, 8)[:, ::2], et, "B must be contiguous"),
            (B, et, "B must be a CUDA tensor")):
        with pytest.raises(RuntimeError, match=msg):
            ops._attn_tbias_table("attention_tbias_forward", badB, bad_et, v, 2)
    with pytest.raises(RuntimeError, match=shape):
        ops._attn_tbias_table("attention_tbias_forward", torch.zeros(3, 1), et, v[:, 0], 2)          # 2-D Q wants 1-D B
    ops_src = open(os.path.join(ROOT, "custom_op_benchmark_amd", "csrc", "torch_ext.cpp")).read()
    for words in ("B must be (n_types) for 2-D Q / K / V, else (n_types, h), got B ",
                  "B must hold at least one type (n_edges = ", "etype must be torch.int32, got ",
                  "etype must be (n_edges) with n_edges = "):
        assert words in ops_src, words
    assert ops_src.count("B must be (n_types) for 2-D Q / K / V") == 1          # stated once


def test_tbias_kernels_census():
    """The exact instantiation sets of the k_attn_tbias_* kernels (nine (H, D) pairs x the template booleans; the generic
    ones per dtype; the replica sum), no scratch and no spilled VGPR in any, static LDS in none (the row pass's table is
    sized at the launch), and names that stay clear of the patterns that pin the kernels of the older ops."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources()
    mine = {n: r for n, r in res.items() if "k_attn_tbias_" in n}
    plain = {"k_attn_tbias_piece_max", "k_attn_tbias_db_reduce"}
    fam = {}
    for n, r in mine.items():
        assert not r["spill_vgpr"] and not r["scratch"] and not r["lds"], (n, r)
        m = re.search(r"graphop::(k_attn_tbias_\w+)<(.*)>\(", n)
        if m:
            fam.setdefault(m.group(1), {})[m.group(2)] = r
        else:
            m = re.search(r"graphop::(k_attn_tbias_\w+)\(", n)
            assert m and m.group(1) in plain, n
            fam.setdefault(m.group(1), {})[""] = r
    hd = ["%d, %d" % p for p in T.HD]
    tf = ("false", "true")
    ty = ("float", "double")
    want = {
        "k_attn_tbias_fwd_rows_f32": {", ".join((a, dr)) for a in hd for dr in tf},
        "k_attn_tbias_bwd_rows_f32": {", ".join((a, c, o, dr)) for a in hd for c in tf for o in tf for dr in tf},
        "k_attn_tbias_pack": {", ".join((a, s)) for a in hd for s in tf},
        "k_attn_tbias_piece_add": set(hd), "k_attn_tbias_piece_fin": set(hd), "k_attn_tbias_piece_max": {""},
        "k_attn_tbias_db_reduce": {""},
        "k_attn_tbias_stats_generic": {", ".join((t, s)) for t in ty for s in tf},
        "k_attn_tbias_fwd_generic": {", ".join((t, s)) for t in ty for s in tf},
        "k_attn_tbias_bwd_row_generic": {", ".join((t, s)) for t in ty for s in tf},
        "k_attn_tbias_bwd_col_generic": {", ".join((t, s)) for t in ty for s in tf},
        "k_attn_tbias_stats_init_generic": set(ty), "k_attn_tbias_stats_fin_generic": set(ty),
        "k_attn_tbias_pack_generic": set(ty),
    }
    assert set(fam) == set(want), sorted(set(fam) ^ set(want))
    for k in want:
        assert set(fam[k]) == want[k], (k, sorted(set(fam[k]) ^ want[k]))
    assert sum(len(v) for v in fam.values()) == len(mine) == 150
    for old in ("k_attn_edge_", "k_attn_etype_", "k_attn_heads_", "k_attn_bias_", "k_attn_weights_"):
        assert not [n for n in mine if old in n], old
    assert not [n for n in mine if re.search(r"k_attn_(bwd_rows|bwd_wown|fwd_walk)_f32<", n)]
    rows = {n: r for n, r in mine.items() if "_rows_f32<" in n}
    assert max(r["vgpr"] for r in rows.values()) <= 256          # two waves per SIMD at least
    print("k_attn_tbias_*_rows_f32 VGPRs: %d..%d" % (min(r["vgpr"] for r in rows.values()), max(r["vgpr"] for r in rows.values())))
    for kind in ("fwd_rows", "bwd_rows"):
        v = [r["vgpr"] for n, r in rows.items() if kind in n]
        print("  %s: %d..%d" % (kind, min(v), max(v)))
    sg = {re.sub(r"^void graphop::|\(.*$", "", n): r["spill_sgpr"] for n, r in mine.items() if r["spill_sgpr"]}
    print("k_attn_tbias_* kernels that spill SGPRs (DESIGN.md 4.5p records them):", sg)


@pytest.mark.parametrize("name", sorted(T.INPUT_SETS))
def test_input_condition(name):
    """Torch's own float32 evaluation of the reference, against the float64 one, stays within 0.5 of the GPU tier's
    bounds (T.tol; dB's with its square-root factor) on every input set that tier uses, with and without dropout: the
    bounds leave a kernel that sums in another order the other half."""
    g, inp, n_types = T.input_set(name)
    src, dst = g.src, g.dst
    nm = T.n_max(inp[4], n_types)
    for p, seed, offset in (T.NONE, T.DROP):
        want = T.reference_step(src, dst, g.n_src, *inp, p, seed, offset)
        got = T.reference_step(src, dst, g.n_src, *inp, p, seed, offset, dtype=torch.float32)
        has = torch.bincount(src, minlength=g.n_src) > 0
        ratios = {k: T.error_ratio(got[k], want[k], **T.tol(torch.float32, p, key=k, n_max=nm)) for k in T.KEYS}
        ratios["stats"] = T.error_ratio(got["stats"][has], want["stats"][has], **T.tol(torch.float32))
        print(name, "p=%g n_max=%d" % (p, nm), {k: round(v, 3) for k, v in ratios.items()})
        assert max(ratios.values()) <= 0.5, (name, p, ratios)
        assert float(AB.biased_scores(src, dst, inp[0], inp[1], T.gathered(inp[3], inp[4])).abs().max()) < 30
