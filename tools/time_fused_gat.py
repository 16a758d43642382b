#!/usr/bin/env python3
"""Time the fused GAT attention step (functions.fused_gat_attention_step: FusedGATAttention, one autograd node, no
E-sized tensor) on the Reddit shape against the composed step (functions.gat_attention_step: GATScores ->
SparseSoftmax -> VectorSPMM).

At full size both steps are first checked against each other: o, del, der and dV, with the error of every node scaled by
that node's magnitude (o, dV: its largest value in the composed result; del, der: a bound of the sum of |terms| behind
it, since del sums to 0 on rows whose scores are all positive).  Then, in one process and alternating, device events time the
fused and the composed fwd+bwd (--warmup untimed rounds, median and min of --iters), and the peak memory each step adds
to what is allocated before it (torch.cuda.max_memory_allocated above the baseline).  A separate profiled round reads
the library's per-launch times of the fused kernels.  One JSON line per (h, d).  Per kernel it names the algorithmic
bytes with the convention of the headline metric (int64 ids at 8 B, values at 4 B, chunk metadata at 16 B per chunk,
node tables once per pass) and, separately, the gathered row bytes E * h * d * 4 of the three passes that gather a
V or dO row per slot (fwd, bwd_row, bwd_col), with the fraction of 8 TB/s each reaches.

--dropout P times the steps with attention dropout instead: the fused dropout step
(functions.fused_gat_attention_dropout_step) against the fused step without dropout, the yardstick, and against the
composed dropout step (functions.gat_attention_dropout_step, which builds and keeps an (E, h) mask), all three
alternating in one process; the check is fused dropout against composed dropout, the per-kernel round that of the
dropout kernels."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from custom_op_benchmark_amd import _lib, functions, graphs  # noqa: E402

PEAK = 8e12


def _timed(fns, warmup, iters):
    """{name: [ms, ...]} of every fn, alternating between them round by round."""
    ev = {n: [] for n in fns}
    for it in range(warmup + iters):
        for n, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            if it >= warmup:
                ev[n].append((a, b))
    torch.cuda.synchronize()
    return {n: [a.elapsed_time(b) for a, b in v] for n, v in ev.items()}


def _node_err(got, want, scale=None):
    """max over nodes (and heads) of |got - want| / the node's magnitude: max |want| of the node, or `scale` (n, h)"""
    n = want.size(0)
    if scale is None:
        g, w = got.double().reshape(n, -1), want.double().reshape(n, -1)
        return float(((g - w).abs().amax(1) / (w.abs().amax(1) + 1e-30)).max())
    diff = (got.double() - want.double()).reshape(n, scale.size(1), -1).abs().amax(-1)
    return float((diff / (scale + 1e-30)).max())


def _grad_scales(g, a, o, V, dO, h, d, mult=1.0):
    """Bounds of the sums behind del and der, per (node, head): sum_j |ds_ij| <= |dO_i| max |V| + |D_i| for del (the
    weights of a row sum to 1), A_j (max |dO| |V_j| + max |D|) for der with A_j = sum_i a_ij.  del sums to 0 where every
    z > 0 (sum_j ds_ij = 0): its own magnitude is no scale.  With dropout every <dO_i, V_j> carries mult = 1 / (1 - p)."""
    V3, dO3, o3 = V.detach().reshape(-1, h, d), dO.reshape(-1, h, d), o.reshape(-1, h, d)
    nV, ndO = V3.double().norm(dim=-1), dO3.double().norm(dim=-1)
    D = (dO3.double() * o3.double()).sum(-1).abs()
    A = torch.zeros_like(nV).index_add_(0, g.dst, a.detach().double().reshape(-1, h))
    return mult * ndO * nV.max() + D, A * (mult * ndO.max() * nV + D.max())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", default="reddit", choices=sorted(graphs.SHAPES))
    ap.add_argument("--hd", default="1x64,8x8,8x32", help="comma-separated h x d pairs")
    ap.add_argument("--slope", type=float, default=0.2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk-size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dropout", type=float, default=0.0, metavar="P", help="time the attention-dropout steps at p = P")
    ap.add_argument("--dropout-seed", type=int, default=1234567890123)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, E = graphs.SHAPES[args.shape]
    g = graphs.chung_lu_graph(N, E, alpha=0.5, seed=args.seed, chunk_size=args.chunk_size, device=dev)
    n_src, n_dst, C_r, C_c = g.n_src, g.n_dst, g.n_row_chunks, g.n_col_chunks
    s = args.slope
    for hd in args.hd.split(","):
        h, d = (int(x) for x in hd.split("x"))
        gen = torch.Generator(device=dev).manual_seed(args.seed + h * 100 + d)
        shp = (lambda n: (n,) if h == 1 else (n, h))
        vs = (lambda n: (n, d) if h == 1 else (n, h, d))
        el = torch.randn(shp(n_src), generator=gen, device=dev).requires_grad_(True)
        er = torch.randn(shp(n_dst), generator=gen, device=dev).requires_grad_(True)
        V = torch.randn(vs(n_dst), generator=gen, device=dev).requires_grad_(True)
        dO = torch.randn(vs(n_src), generator=gen, device=dev)
        leaves = (el, er, V)

        def fused():
            for x in leaves:
                x.grad = None
            return functions.fused_gat_attention_step(g, el, er, V, dO, s)

        def composed():
            for x in leaves:
                x.grad = None
            return functions.gat_attention_step(g, el, er, V, dO, s)

        nodrop = None
        if args.dropout > 0:      # the dropout forms take the places of the two steps; the undropped fused step stays
            nodrop, drop = fused, (args.dropout, args.dropout_seed, 7)

            def fused():
                for x in leaves:
                    x.grad = None
                return functions.fused_gat_attention_dropout_step(g, el, er, V, dO, *drop, s)

            def composed():
                for x in leaves:
                    x.grad = None
                return functions.gat_attention_dropout_step(g, el, er, V, dO, *drop, s)

        # full-size check (also builds and caches the plans both steps use)
        _, a_c, o_c = composed()
        o_c = o_c.detach()
        want = [o_c] + [x.grad.clone() for x in leaves]
        sc_l, sc_r = _grad_scales(g, a_c, o_c, V, dO, h, d, 1.0 / (1.0 - args.dropout))
        del a_c
        o_f = fused().detach()
        got = [o_f] + [x.grad.clone() for x in leaves]
        torch.cuda.synchronize()
        err = {n: _node_err(x, y, sc) for n, x, y, sc in zip(("o", "del", "der", "dV"), got, want,
                                                              (None, sc_l, sc_r, None))}
        assert all(v < 1e-4 for v in err.values()), err
        del o_c, o_f, want, got, sc_l, sc_r

        # peak memory each step adds to what is allocated before it
        peak = {}
        for name, fn in (("fused", fused), ("composed", composed)) + ((("fused_no_dropout", nodrop),) if nodrop else ()):
            for x in leaves:
                x.grad = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = fn()
            torch.cuda.synchronize()
            peak[name] = torch.cuda.max_memory_allocated() - base
            del out

        fns = {"fused_fwd_bwd": fused, "composed_fwd_bwd": composed}
        if nodrop:
            fns["fused_no_dropout_fwd_bwd"] = nodrop
        t = _timed(fns, args.warmup, args.iters)
        timings = {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)} for n, v in t.items()}

        # per-kernel times from the library's launch profile, in a round of their own
        _lib.profile_enable(True)
        try:
            _lib.profile_read()
            for _ in range(args.iters):
                fused()
            torch.cuda.synchronize()
            prof = _lib.profile_read()
        finally:
            _lib.profile_enable(False)
        nh_l, nh_r = n_src * h * 4, n_dst * h * 4            # one per-(node, head) scalar table
        row_l, row_r = n_src * h * d * 4, n_dst * h * d * 4   # one node-row table
        ids_r, ids_c = E * 8 + 16 * C_r, E * 8 + 16 * C_c
        gathered = E * h * d * 4
        model = {   # tag: (algorithmic bytes, gathered row bytes)
            "gat_attn_stats": (ids_r + nh_l + nh_r + 2 * nh_l, 0),
            "gat_attn_fwd": (ids_r + nh_l + 2 * nh_l + nh_r + row_r + row_l, gathered),
            "gat_attn_pack": (nh_l + 2 * nh_l + 2 * row_l + 4 * nh_l, 0),
            "gat_attn_bwd_row": (ids_r + row_l + 4 * nh_l + nh_r + row_r + nh_l, gathered),
            "gat_attn_bwd_col": (ids_c + row_r + nh_r + 4 * nh_l + row_l + nh_r + row_r, gathered),
        }
        dtag = {"gat_attn_fwd": "gat_attn_drop_fwd", "gat_attn_bwd_row": "gat_attn_drop_bwd_row",
                "gat_attn_bwd_col": "gat_attn_drop_bwd_col"} if nodrop else {}
        kernels = {}
        for tag, (nbytes, gb) in model.items():
            tag = dtag.get(tag, tag)      # the dropout forms read the same bytes
            p = prof[tag]
            sec = p["mean_ms"] * 1e-3
            kernels[tag] = {"kernel": p["kernel"], "calls": p["calls"], "mean_ms": round(p["mean_ms"], 4),
                            "min_ms": round(p["min_ms"], 4), "algorithmic_bytes": nbytes,
                            "fraction_of_8TBs": round(nbytes / sec / PEAK, 3)}
            if gb:
                kernels[tag]["gathered_row_bytes"] = gb
                kernels[tag]["gathered_fraction_of_8TBs"] = round(gb / sec / PEAK, 3)
        f, c = timings["fused_fwd_bwd"]["median_ms"], timings["composed_fwd_bwd"]["median_ms"]
        extra = {}
        if nodrop:
            extra = {"dropout": {"p": drop[0], "seed": drop[1], "offset": drop[2]},
                     "fused_dropout_over_fused_no_dropout":
                         round(f / timings["fused_no_dropout_fwd_bwd"]["median_ms"], 3)}
        print(json.dumps({
            "tool": "tools/time_fused_gat.py", "shape": args.shape, "n_src": n_src, "n_dst": n_dst, "n_edges": E,
            "row_chunks": C_r, "col_chunks": C_c, "chunk_size": args.chunk_size, "h": h, "d": d, "negative_slope": s,
            "warmup": args.warmup, "iters": args.iters, "node_scaled_error_vs_composed": err, "timings": timings,
            "fused_over_composed": round(f / c, 3), "peak_added_bytes": peak,
            "one_edge_tensor_bytes": E * h * 4, "kernels": kernels, **extra,
            "device": torch.cuda.get_device_name(dev)}),
            flush=True)
        del el, er, V, dO, leaves
        torch.cuda.empty_cache()
    _lib.check_errors()


if __name__ == "__main__":
    main()
