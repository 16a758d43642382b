#!/usr/bin/env python3
"""Time the fused GAT attention step with an edge term (functions.fused_gat_edge_attention_step: FusedGATEdgeAttention,
s = LeakyReLU(el[i] + er[j] + ee[e]); the gradient of ee is the only E-sized tensor made) on the Reddit shape against
two other steps, all three alternating in one process:
  fused_no_edge - functions.fused_gat_attention_step, the layer without the edge term: the yardstick
  composed      - functions.gat_edge_attention_step: GATScores at slope 1 -> + ee -> leaky_relu -> SparseSoftmax ->
                  VectorSPMM, which keeps z, z + ee, s and a and makes as many gradients.

At full size the fused and the composed edge steps are first checked against each other: o, del, der, dee and dV, with
the error of every node scaled by that node's magnitude as in tools/time_fused_gat.py (dee: by the bound of its row's
sum of |ds|).  Then device events time the three fwd+bwd (--warmup untimed rounds, median and min of --iters), and the
peak memory each step adds to what is allocated before it.  A separate profiled round reads the library's per-launch
times of the fused edge kernels and of the fused kernels without the edge term.  One JSON line per (h, d).  Per kernel
it names the algorithmic bytes with the convention of the headline metric: those of tools/time_fused_gat.py plus, in
each of stats, fwd, bwd_row and bwd_col, E * h * 4 for ee and E * 8 for eid, plus E * h * 4 for the dee store in
bwd_row.

--dropout P runs all three steps at p = P (the composed one builds and keeps an (E, h) mask); --permute-ids renumbers
the edges at random, so the row-major passes read eid as well (graph_from_coo yields eid_r = arange(E), which they
skip); --fixed-ee times the fused step with ee not requiring grad (no dee)."""
import argparse
import dataclasses
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from custom_op_benchmark_amd import _lib, functions, graphs  # noqa: E402
from time_fused_gat import PEAK, _grad_scales, _node_err, _timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", default="reddit", choices=sorted(graphs.SHAPES))
    ap.add_argument("--hd", default="1x64,8x8,8x32", help="comma-separated h x d pairs")
    ap.add_argument("--slope", type=float, default=0.2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk-size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dropout", type=float, default=0.0, metavar="P", help="run the three steps at p = P")
    ap.add_argument("--dropout-seed", type=int, default=1234567890123)
    ap.add_argument("--permute-ids", action="store_true", help="renumber the edges at random")
    ap.add_argument("--fixed-ee", action="store_true", help="ee does not require grad in the fused step (no dee)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, E = graphs.SHAPES[args.shape]
    g = graphs.chung_lu_graph(N, E, alpha=0.5, seed=args.seed, chunk_size=args.chunk_size, device=dev)
    src_e = g.src
    if args.permute_ids:
        perm = torch.randperm(E, generator=torch.Generator(device=dev).manual_seed(args.seed + 1), device=dev)
        src_e, dst_e = torch.empty_like(g.src), torch.empty_like(g.dst)
        src_e[perm], dst_e[perm] = g.src, g.dst           # the edge list in the new edge-id order
        g = dataclasses.replace(g, src=src_e, dst=dst_e, eid_r=perm[g.eid_r], eid_c=perm[g.eid_c])
    n_src, n_dst, C_r, C_c = g.n_src, g.n_dst, g.n_row_chunks, g.n_col_chunks
    s = args.slope
    drop = (args.dropout, args.dropout_seed if args.dropout > 0 else 0, 7 if args.dropout > 0 else 0)
    for hd in args.hd.split(","):
        h, d = (int(x) for x in hd.split("x"))
        gen = torch.Generator(device=dev).manual_seed(args.seed + h * 100 + d)
        shp = (lambda n: (n,) if h == 1 else (n, h))
        vs = (lambda n: (n, d) if h == 1 else (n, h, d))
        el = torch.randn(shp(n_src), generator=gen, device=dev).requires_grad_(True)
        er = torch.randn(shp(n_dst), generator=gen, device=dev).requires_grad_(True)
        V = torch.randn(vs(n_dst), generator=gen, device=dev).requires_grad_(True)
        dO = torch.randn(vs(n_src), generator=gen, device=dev)
        ee = torch.randn(shp(E), generator=gen, device=dev).requires_grad_(True)
        ee_fixed = ee.detach()
        leaves = (el, er, ee, V)

        def clear():
            for x in leaves:
                x.grad = None

        def fused():
            clear()
            return functions.fused_gat_edge_attention_step(g, el, er, ee_fixed if args.fixed_ee else ee, V, dO, s, *drop)

        def composed():
            clear()
            return functions.gat_edge_attention_step(g, el, er, ee, V, dO, s, *drop)

        def no_edge():
            clear()
            if args.dropout > 0:
                return functions.fused_gat_attention_dropout_step(g, el, er, V, dO, *drop, s)
            return functions.fused_gat_attention_step(g, el, er, V, dO, s)

        # full-size check (also builds and caches the plans the steps use)
        _, a_c, o_c = composed()
        o_c = o_c.detach()
        want = [o_c] + [x.grad.clone() for x in leaves]
        sc_l, sc_r = _grad_scales(g, a_c, o_c, V, dO, h, d, 1.0 / (1.0 - args.dropout))
        del a_c
        o_f = fused().detach()
        got = [o_f] + [x.grad.clone() if x.grad is not None else None for x in leaves]
        torch.cuda.synchronize()
        err = {n: _node_err(x, y, sc) for n, x, y, sc in zip(("o", "del", "der", "dee", "dV"), got, want,
                                                              (None, sc_l, sc_r, None, None)) if n != "dee"}
        if got[3] is not None:
            diff = (got[3].double() - want[3].double()).reshape(E, h).abs()
            err["dee"] = float((diff / (sc_l[src_e] + 1e-30)).max())
        assert all(v < 1e-4 for v in err.values()), err
        del o_c, o_f, want, got, sc_l, sc_r

        # peak memory each step adds to what is allocated before it
        peak = {}
        for name, fn in (("fused", fused), ("composed", composed), ("fused_no_edge", no_edge)):
            clear()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = fn()
            torch.cuda.synchronize()
            peak[name] = torch.cuda.max_memory_allocated() - base
            del out
        clear()

        t = _timed({"fused_fwd_bwd": fused, "fused_no_edge_fwd_bwd": no_edge, "composed_fwd_bwd": composed},
                   args.warmup, args.iters)
        timings = {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)} for n, v in t.items()}

        # per-kernel times from the library's launch profile, in a round of their own
        _lib.profile_enable(True)
        try:
            _lib.profile_read()
            for _ in range(args.iters):
                fused()
                no_edge()
            torch.cuda.synchronize()
            prof = _lib.profile_read()
        finally:
            _lib.profile_enable(False)
        nh_l, nh_r = n_src * h * 4, n_dst * h * 4            # one per-(node, head) scalar table
        row_l, row_r = n_src * h * d * 4, n_dst * h * d * 4   # one node-row table
        ids_r, ids_c = E * 8 + 16 * C_r, E * 8 + 16 * C_c
        gathered = E * h * d * 4
        edge = E * h * 4 + E * 8                              # ee and eid of a pass
        dee = 0 if args.fixed_ee else E * h * 4
        model = {   # pass: (algorithmic bytes without the edge term, the edge term's, gathered row bytes)
            "stats": (ids_r + nh_l + nh_r + 2 * nh_l, edge, 0),
            "fwd": (ids_r + nh_l + 2 * nh_l + nh_r + row_r + row_l, edge, gathered),
            "pack": (nh_l + 2 * nh_l + 2 * row_l + 4 * nh_l, 0, 0),
            "bwd_row": (ids_r + row_l + 4 * nh_l + nh_r + row_r + nh_l, edge + dee, gathered),
            "bwd_col": (ids_c + row_r + nh_r + 4 * nh_l + row_l + nh_r + row_r, edge, gathered),
        }
        dropped = args.dropout > 0
        kernels = {}
        for name, (base_bytes, edge_bytes, gb) in model.items():
            dname = "drop_" + name if dropped and name in ("fwd", "bwd_row", "bwd_col") else name
            for op, nbytes in (("gat_edge_attn_", base_bytes + edge_bytes), ("gat_attn_", base_bytes)):
                p = prof[op + dname]
                sec = p["mean_ms"] * 1e-3
                kernels[op + dname] = {"kernel": p["kernel"], "calls": p["calls"], "mean_ms": round(p["mean_ms"], 4),
                                       "min_ms": round(p["min_ms"], 4), "algorithmic_bytes": nbytes,
                                       "fraction_of_8TBs": round(nbytes / sec / PEAK, 3)}
                if gb:
                    kernels[op + dname]["gathered_row_bytes"] = gb
                    kernels[op + dname]["gathered_fraction_of_8TBs"] = round(gb / sec / PEAK, 3)
        extra_ms = {n: round(kernels["gat_edge_attn_" + n]["mean_ms"] - kernels["gat_attn_" + n]["mean_ms"], 4)
                    for n in (("drop_" if dropped else "") + x for x in ("fwd", "bwd_row", "bwd_col"))}
        extra_ms["stats"] = round(kernels["gat_edge_attn_stats"]["mean_ms"] - kernels["gat_attn_stats"]["mean_ms"], 4)
        total_extra = sum(extra_ms.values())
        col = extra_ms[("drop_" if dropped else "") + "bwd_col"]
        f, c, n = (timings[k]["median_ms"] for k in ("fused_fwd_bwd", "composed_fwd_bwd", "fused_no_edge_fwd_bwd"))
        print(json.dumps({
            "tool": "tools/time_fused_gat_edge.py", "shape": args.shape, "n_src": n_src, "n_dst": n_dst, "n_edges": E,
            "row_chunks": C_r, "col_chunks": C_c, "chunk_size": args.chunk_size, "h": h, "d": d, "negative_slope": s,
            "warmup": args.warmup, "iters": args.iters, "permuted_edge_ids": args.permute_ids,
            "ee_requires_grad": not args.fixed_ee, "dropout": {"p": drop[0], "seed": drop[1], "offset": drop[2]},
            "node_scaled_error_vs_composed": err, "timings": timings,
            "fused_edge_over_fused_no_edge": round(f / n, 3), "fused_edge_over_composed_edge": round(f / c, 3),
            "peak_added_bytes": peak, "one_edge_tensor_bytes": E * h * 4, "kernels": kernels,
            "extra_kernel_ms_over_no_edge": extra_ms,
            "bwd_col_share_of_extra_kernel_ms": round(col / total_extra, 3) if total_extra > 0 else None,
            "device": torch.cuda.get_device_name(dev)}),
            flush=True)
        del el, er, ee, ee_fixed, V, dO, leaves
        torch.cuda.empty_cache()
    _lib.check_errors()


if __name__ == "__main__":
    main()
