#!/usr/bin/env python3
"""Time the fused GATv2 attention step (functions.fused_gatv2_attention_step: FusedGATv2Attention, one autograd node, no
E-sized tensor) on the Reddit shape against the composed step (functions.gatv2_attention_step with V=None: GATv2Scores
-> SparseSoftmax -> VectorSPMM over xr).

At full size both steps are first compared: o, dxl, dxr with the error of every node scaled by the node's largest value in
the composed result, datt (and with --edge dxe) by its own largest value.  Then, in one process and alternating, device events time the fused
and the composed fwd+bwd (--warmup untimed rounds, median and min of --iters), and the peak memory each step adds to
what is allocated before it (torch.cuda.max_memory_allocated above the baseline).  The only assertion is the memory
condition: the fused step adds less than one (E, h) fp32 tensor, the composed one more than two.  Separate profiled
rounds read the library's per-launch times: the fused kernels, and the yardsticks k_gatv2_fwd_f32 (from the composed
step) and k_gat_attn_bwd_row_f32 (from the fused GAT v1 step) at the same (h, d).  Per gather pass the record names the
algorithmic bytes (ids 8 E + 16 C, node tables once) and the gathered row bytes (E * h * d * 4 per row gather: one in
the forward and the row pass, two in the column pass) with the fraction of 8 TB/s each reaches.
One JSON record per (h, d), printed and collected in --out (default profiles/fused_gatv2_bench.json).

--dropout P times the steps with attention dropout instead: the fused dropout step
(functions.fused_gatv2_attention_dropout_step) against the fused step without dropout, the yardstick, and against the
composed dropout step (functions.gatv2_attention_dropout_step, which builds and keeps an (E, h) mask), all three
alternating in one process; the comparison is fused dropout against composed dropout, the memory condition asks the
composed step for more than three (E, h) tensors, and the per-kernel rounds are those of the dropout kernels and of the
undropped fused kernels (the yardstick kernels of the other ops are left out).  --out then defaults to
profiles/fused_gatv2_dropout_bench.json.

--edge times the layer with edge features instead: three steps alternate in one process, the fused
edge step (functions.fused_gatv2_edge_attention_step), the fused dropout step without xe (yardstick 1) and the composed
edge step (functions.gatv2_edge_attention_step, yardstick 2; --no-composed leaves it out where its (E, h, d)
temporaries do not fit).  --dropout P applies to all three (default 0).  Reported: median and min, the peak memory each
step adds, and per kernel the time with the bytes of the model of 4.5i: every pass streams E h d 4 bytes of xe and 8 E
of eid (none where the row-major plan says eid_identity), the row pass writes E h d 4 of dxe.  --edges N replaces the
shape's edge count (the record names the graph).  Nothing is asserted on a time.  --out defaults to
profiles/fused_gatv2_edge_bench.json."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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


def _node_err(got, want):
    """max over nodes of |got - want| / the node's largest |want|"""
    n = want.size(0)
    g, w = got.double().reshape(n, -1), want.double().reshape(n, -1)
    return float(((g - w).abs().amax(1) / (w.abs().amax(1) + 1e-30)).max())


def _profile(fn, iters):
    _lib.profile_enable(True)
    try:
        _lib.profile_read()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return _lib.profile_read()
    finally:
        _lib.profile_enable(False)


def edge_records(args, g, dev):
    """the records of --edge, one per (h, d)"""
    E, n_src, n_dst, C_r, C_c = g.n_edges, g.n_src, g.n_dst, g.n_row_chunks, g.n_col_chunks
    s, drop = args.slope, (args.dropout, args.dropout_seed, 7)
    identity = bool(_lib.get_plan(g.row, g.ptr_r, g.eid_r, g.indices_r, n_dst).info.eid_identity)
    records = []
    for hd in args.hd.split(","):
        h, d = (int(x) for x in hd.split("x"))
        gen = torch.Generator(device=dev).manual_seed(args.seed + h * 100 + d)
        ns = (lambda n: (n, d) if h == 1 else (n, h, d))
        xl = torch.randn(ns(n_src), generator=gen, device=dev).requires_grad_(True)
        xr = torch.randn(ns(n_dst), generator=gen, device=dev).requires_grad_(True)
        xe = torch.randn(ns(E), generator=gen, device=dev).requires_grad_(True)
        att = (torch.randn(ns(1)[1:], generator=gen, device=dev) / d ** 0.5).requires_grad_(True)
        dO = torch.randn(ns(n_src), generator=gen, device=dev)
        leaves = (xl, xr, xe, att)

        def clear():
            for x in leaves:
                x.grad = None

        def fused_edge():
            clear()
            return functions.fused_gatv2_edge_attention_step(g, xl, xr, xe, att, dO, s, *drop)

        def fused_no_edge():
            clear()
            return functions.fused_gatv2_attention_dropout_step(g, xl, xr, att, dO, *drop, s)

        def composed_edge():
            clear()
            return functions.gatv2_edge_attention_step(g, xl, xr, xe, att, dO, s, *drop)

        fns = {"fused_edge_fwd_bwd": fused_edge, "fused_no_edge_fwd_bwd": fused_no_edge}
        if not args.no_composed:
            fns["composed_edge_fwd_bwd"] = composed_edge
        err = None
        if not args.no_composed:      # full-size comparison (also builds and caches the plans)
            o_c = composed_edge()[2].detach()
            want = [o_c] + [x.grad.clone() for x in leaves]
            o_f = fused_edge().detach()
            got = [o_f] + [x.grad.clone() for x in leaves]
            torch.cuda.synchronize()
            err = {n: _node_err(x, y) for n, x, y in zip(("o", "dxl", "dxr"), got, want)}
            for n, k in (("dxe", 3), ("datt", 4)):      # by the tensor's largest value: an edge's own row may be ~0
                err[n] = float((got[k] - want[k]).abs().max() / want[k].abs().max())
            del o_c, o_f, want, got
        peak = {}
        for name, fn in fns.items():
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
        t = _timed(fns, args.warmup, args.iters)
        timings = {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)} for n, v in t.items()}
        prof = _profile(fused_edge, args.iters)
        prof0 = _profile(fused_no_edge, args.iters)
        nh_l = n_src * h * 4
        row_l, row_r = n_src * h * d * 4, n_dst * h * d * 4
        ids_r, ids_c = E * 8 + 16 * C_r, E * 8 + 16 * C_c
        rows = E * h * d * 4                                    # one (E, h, d) stream: a row gather, xe or dxe
        eid_r = 0 if identity else 8 * E
        dropped = args.dropout > 0
        tags = {"fwd": "gv2edge_drop_fwd" if dropped else "gv2edge_fwd",
                "bwd_row": "gv2edge_drop_bwd_row" if dropped else "gv2edge_bwd_row",
                "bwd_col": "gv2edge_drop_bwd_col" if dropped else "gv2edge_bwd_col"}
        model = {   # pass: (algorithmic bytes without the gathers, row gathers per slot, edge-stream bytes)
            "fwd": (ids_r + row_l + row_r + row_l + 2 * nh_l, 1, rows + eid_r),
            "bwd_row": (ids_r + 2 * row_l + 4 * nh_l + row_r + row_l, 1, 2 * rows + eid_r),
            "bwd_col": (ids_c + row_r + 2 * row_l + 4 * nh_l + row_r, 2, rows + 8 * E),
        }
        kernels = {}
        for name, (nbytes, gathers, edge_bytes) in model.items():
            q = prof[tags[name]]
            q0 = prof0.get(tags[name].replace("gv2edge", "gv2attn"))
            sec = q["mean_ms"] * 1e-3
            kernels[tags[name]] = {
                "kernel": q["kernel"], "calls": q["calls"], "mean_ms": round(q["mean_ms"], 4),
                "min_ms": round(q["min_ms"], 4), "algorithmic_bytes": nbytes, "gathered_row_bytes": gathers * rows,
                "edge_stream_bytes": edge_bytes,
                "edge_stream_fraction_of_8TBs": round(edge_bytes / sec / PEAK, 3),
                "all_bytes_fraction_of_8TBs": round((nbytes + gathers * rows + edge_bytes) / sec / PEAK, 3),
                "no_edge_mean_ms": round(q0["mean_ms"], 4) if q0 else None}
        for tag in ("gv2attn_pack", "gv2attn_datt_fin"):
            kernels[tag] = {"kernel": prof[tag]["kernel"], "mean_ms": round(prof[tag]["mean_ms"], 4)}
        f = timings["fused_edge_fwd_bwd"]["median_ms"]
        rec = {
            "tool": "tools/time_fused_gatv2.py --edge", "graph": "chung_lu_graph(%d, %d, alpha=0.5, seed=%d)" % (
                n_src, E, args.seed), "shape": args.shape, "n_src": n_src, "n_dst": n_dst, "n_edges": E,
            "row_chunks": C_r, "col_chunks": C_c, "chunk_size": args.chunk_size, "h": h, "d": d, "negative_slope": s,
            "dropout": {"p": drop[0], "seed": drop[1], "offset": drop[2]}, "eid_identity": identity,
            "warmup": args.warmup, "iters": args.iters, "node_scaled_difference_vs_composed": err, "timings": timings,
            "fused_edge_over_fused_no_edge": round(f / timings["fused_no_edge_fwd_bwd"]["median_ms"], 3),
            "fused_edge_over_composed_edge": (round(f / timings["composed_edge_fwd_bwd"]["median_ms"], 3)
                                              if not args.no_composed else None),
            "peak_added_bytes": peak, "one_edge_row_tensor_bytes": rows, "kernels": kernels,
            "device": torch.cuda.get_device_name(dev)}
        print(json.dumps(rec), flush=True)
        records.append(rec)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:      # rewritten after every shape: a run that is cut short keeps what it has
            json.dump(records, fh, indent=1)
            fh.write("\n")
        del xl, xr, xe, att, dO, leaves
        torch.cuda.empty_cache()
    _lib.check_errors()


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
    ap.add_argument("--edge", action="store_true", help="time the layer with edge features (xe) instead")
    ap.add_argument("--edges", type=int, default=None, metavar="N", help="with --edge: N edges instead of the shape's")
    ap.add_argument("--no-composed", action="store_true", help="with --edge: leave the composed edge step out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "fused_gatv2_edge_bench.json" if args.edge else
                                "fused_gatv2_dropout_bench.json" if args.dropout > 0 else "fused_gatv2_bench.json")
    dev = torch.device("cuda:0")
    N, E = graphs.SHAPES[args.shape]
    if args.edge and args.edges:
        E = args.edges
    g = graphs.chung_lu_graph(N, E, alpha=0.5, seed=args.seed, chunk_size=args.chunk_size, device=dev)
    if args.edge:
        return edge_records(args, g, dev)
    n_src, n_dst, C_r, C_c = g.n_src, g.n_dst, g.n_row_chunks, g.n_col_chunks
    s = args.slope
    records = []
    for hd in args.hd.split(","):
        h, d = (int(x) for x in hd.split("x"))
        gen = torch.Generator(device=dev).manual_seed(args.seed + h * 100 + d)
        ns = (lambda n: (n, d) if h == 1 else (n, h, d))
        xl = torch.randn(ns(n_src), generator=gen, device=dev).requires_grad_(True)
        xr = torch.randn(ns(n_dst), generator=gen, device=dev).requires_grad_(True)
        att = (torch.randn(ns(1)[1:], generator=gen, device=dev) / d ** 0.5).requires_grad_(True)
        dO = torch.randn(ns(n_src), generator=gen, device=dev)
        leaves = (xl, xr, att)

        def fused():
            for x in leaves:
                x.grad = None
            return functions.fused_gatv2_attention_step(g, xl, xr, att, dO, s)

        def composed():
            for x in leaves:
                x.grad = None
            return functions.gatv2_attention_step(g, xl, xr, att, dO, s)

        nodrop = None
        if args.dropout > 0:      # the dropout forms take the places of the two steps; the undropped fused step stays
            nodrop, drop = fused, (args.dropout, args.dropout_seed, 7)

            def fused():
                for x in leaves:
                    x.grad = None
                return functions.fused_gatv2_attention_dropout_step(g, xl, xr, att, dO, *drop, s)

            def composed():
                for x in leaves:
                    x.grad = None
                return functions.gatv2_attention_dropout_step(g, xl, xr, att, dO, *drop, s)

        # full-size comparison (also builds and caches the plans both steps use)
        o_c = composed()[2].detach()
        want = [o_c] + [x.grad.clone() for x in leaves]
        o_f = fused().detach()
        got = [o_f] + [x.grad.clone() for x in leaves]
        torch.cuda.synchronize()
        err = {n: _node_err(x, y) for n, x, y in zip(("o", "dxl", "dxr"), got, want)}
        err["datt"] = float((got[3].double() - want[3].double()).abs().max() / want[3].double().abs().max())
        del o_c, o_f, want, got

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
        edge_tensor = E * h * 4
        assert peak["fused"] < edge_tensor, (peak, edge_tensor)
        assert peak["composed"] > (3 if nodrop else 2) * edge_tensor, (peak, edge_tensor)

        fns = {"fused_fwd_bwd": fused, "composed_fwd_bwd": composed}
        if nodrop:
            fns["fused_no_dropout_fwd_bwd"] = nodrop
        t = _timed(fns, args.warmup, args.iters)
        timings = {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)} for n, v in t.items()}

        # per-kernel times from the library's launch profile, in rounds of their own
        prof = _profile(fused, args.iters)
        prof_c = prof_v1 = {}
        if not nodrop:      # the yardstick kernels of the other ops belong to the undropped record
            prof_c = _profile(composed, args.iters)
            el = torch.randn((n_src,) if h == 1 else (n_src, h), generator=gen, device=dev).requires_grad_(True)
            er = torch.randn((n_dst,) if h == 1 else (n_dst, h), generator=gen, device=dev).requires_grad_(True)
            V = xr.detach().clone().requires_grad_(True)

            def gat_v1():
                for x in (el, er, V):
                    x.grad = None
                return functions.fused_gat_attention_step(g, el, er, V, dO, s)
            prof_v1 = _profile(gat_v1, args.iters)
            del el, er, V
        nh_l = n_src * h * 4                                  # one per-(node, head) scalar table
        row_l, row_r = n_src * h * d * 4, n_dst * h * d * 4   # one node-row table
        ids_r, ids_c = E * 8 + 16 * C_r, E * 8 + 16 * C_c
        gathered = E * h * d * 4
        model = {   # tag: (algorithmic bytes, row gathers per slot)
            "gv2attn_fwd": (ids_r + row_l + row_r + row_l + 2 * nh_l, 1),
            "gv2attn_pack": (2 * nh_l + 2 * row_l + 4 * nh_l, 0),
            "gv2attn_bwd_row": (ids_r + 2 * row_l + 4 * nh_l + row_r + row_l, 1),
            "gv2attn_bwd_col": (ids_c + row_r + 2 * row_l + 4 * nh_l + row_r, 2),
            "gv2attn_datt_fin": (0, 0),
        }
        dtag = {"gv2attn_fwd": "gv2attn_drop_fwd", "gv2attn_bwd_row": "gv2attn_drop_bwd_row",
                "gv2attn_bwd_col": "gv2attn_drop_bwd_col"} if nodrop else {}
        kernels = {}
        for tag, (nbytes, gathers) in model.items():
            tag = dtag.get(tag, tag)      # the dropout forms read the same bytes
            p = prof[tag]
            sec = p["mean_ms"] * 1e-3
            kernels[tag] = {"kernel": p["kernel"], "calls": p["calls"], "mean_ms": round(p["mean_ms"], 4),
                            "min_ms": round(p["min_ms"], 4)}
            if nbytes:
                kernels[tag]["algorithmic_bytes"] = nbytes
                kernels[tag]["fraction_of_8TBs"] = round(nbytes / sec / PEAK, 3)
            if gathers:
                kernels[tag]["gathered_row_bytes"] = gathers * gathered
                kernels[tag]["gathered_fraction_of_8TBs"] = round(gathers * gathered / sec / PEAK, 3)
        yard = {}
        for tag, p in (("gatv2_fwd", prof_c.get("gatv2_fwd")), ("gatv2_bwd_row", prof_c.get("gatv2_bwd_row")),
                       ("gatv2_bwd_col", prof_c.get("gatv2_bwd_col")), ("gat_attn_fwd", prof_v1.get("gat_attn_fwd")),
                       ("gat_attn_bwd_row", prof_v1.get("gat_attn_bwd_row")),
                       ("gat_attn_bwd_col", prof_v1.get("gat_attn_bwd_col"))):
            if p:
                yard[tag] = {"kernel": p["kernel"], "mean_ms": round(p["mean_ms"], 4), "min_ms": round(p["min_ms"], 4),
                             "gathered_fraction_of_8TBs": round(gathered / (p["mean_ms"] * 1e-3) / PEAK, 3)}
        f, c = timings["fused_fwd_bwd"]["median_ms"], timings["composed_fwd_bwd"]["median_ms"]
        extra = {"yardstick_kernels": yard}
        if nodrop:
            extra = {"dropout": {"p": drop[0], "seed": drop[1], "offset": drop[2]},
                     "fused_dropout_over_fused_no_dropout":
                         round(f / timings["fused_no_dropout_fwd_bwd"]["median_ms"], 3),
                     "kernels_no_dropout": {tag: {"kernel": p["kernel"], "mean_ms": round(p["mean_ms"], 4),
                                                  "min_ms": round(p["min_ms"], 4)}
                                            for tag, p in _profile(nodrop, args.iters).items() if tag in model}}
        rec = {
            "tool": "tools/time_fused_gatv2.py", "shape": args.shape, "n_src": n_src, "n_dst": n_dst, "n_edges": E,
            "row_chunks": C_r, "col_chunks": C_c, "chunk_size": args.chunk_size, "h": h, "d": d, "negative_slope": s,
            "warmup": args.warmup, "iters": args.iters, "node_scaled_difference_vs_composed": err, "timings": timings,
            "fused_over_composed": round(f / c, 3), "peak_added_bytes": peak, "one_edge_tensor_bytes": edge_tensor,
            "kernels": kernels, **extra, "device": torch.cuda.get_device_name(dev)}
        print(json.dumps(rec), flush=True)
        records.append(rec)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:      # rewritten after every shape: a run that is cut short keeps what it has
            json.dump(records, fh, indent=1)
            fh.write("\n")
        del xl, xr, att, dO, leaves
        torch.cuda.empty_cache()
    _lib.check_errors()


if __name__ == "__main__":
    main()
