#!/usr/bin/env python3
"""Time the fused dot-product attention step with edge features (functions.fused_attention_edge_step: FusedAttentionEdge,
one autograd node, nothing edge-sized but xe and dxe).

Three steps alternate in one process, --warmup untimed rounds and then --iters rounds timed by device events:
  edge      the fused edge step;
  no_edge   functions.fused_attention_bias_step with the knobs attn_heads = 1 and attn_rows = 1: the same chunk-driver
            family without xe (its edge-sized operands are the (E, h) bias and its gradient);
  composed  functions.attention_edge_step: torch index_selects, + xe[eid], SparseSoftmax, the mask of edge_dropout_mask,
            a segment sum (--no-composed leaves it out where its (E, h, d) temporaries do not fit; a shape on which it
            runs out of memory is recorded as such).
Reported per (h, d) and p: medians (min..max), the peak memory each step adds to what is allocated before it, the
per-pass kernel times of the library's launch profile (rounds of their own) next to the bytes of the model of 4.5m -- per
pass those of 4.5l plus 4 E h d of xe as a stream, 8 E of eid unless the row-major plan says identity (the column pass
always pays it), and 4 E h d of dxe in the row pass -- and the largest node-scaled error of the fused step against the
composed one (dxe by the tensor's largest value).  Nothing is asserted on a time.
Graph: chung_lu_graph(N of --shape, --edges or the shape's E, alpha=0.5, seed=--seed).  One JSON record per case, printed
and collected in --out (default profiles/fused_attention_edge_bench.json; --append keeps the records already there)."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", default="reddit", choices=sorted(graphs.SHAPES))
    ap.add_argument("--edges", type=int, default=None, metavar="N", help="N edges instead of the shape's")
    ap.add_argument("--hd", default="1x64,8x8,8x32", help="comma-separated h x d pairs")
    ap.add_argument("--dropout", default="0,0.3", help="comma-separated dropout probabilities")
    ap.add_argument("--dropout-seed", type=int, default=1234567890123)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk-size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-composed", action="store_true", help="leave the composed edge step out")
    ap.add_argument("--append", action="store_true", help="keep the records --out already holds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_attention_edge_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, E = graphs.SHAPES[args.shape]
    if args.edges:
        E = args.edges
    g = graphs.chung_lu_graph(N, E, alpha=0.5, seed=args.seed, chunk_size=args.chunk_size, device=dev)
    E, n_q, n_k, C_r, C_c = g.n_edges, g.n_src, g.n_dst, g.n_row_chunks, g.n_col_chunks
    identity = bool(_lib.get_plan(g.row, g.ptr_r, g.eid_r, g.indices_r, n_k).info.eid_identity)
    records = []
    if args.append and os.path.exists(args.out):
        with open(args.out) as fh:
            records = json.load(fh)
    _lib.tune("attn_heads", 1)
    _lib.tune("attn_rows", 1)
    for hd in args.hd.split(","):
        h, d = (int(x) for x in hd.split("x"))
        gen = torch.Generator(device=dev).manual_seed(args.seed + h * 100 + d)
        ns = (lambda n: (n, d) if h == 1 else (n, h, d))
        Q = (torch.randn(ns(n_q), generator=gen, device=dev) / d ** 0.5).requires_grad_(True)
        K = torch.randn(ns(n_k), generator=gen, device=dev).requires_grad_(True)
        V = torch.randn(ns(n_k), generator=gen, device=dev).requires_grad_(True)
        xe = torch.randn(ns(E), generator=gen, device=dev).requires_grad_(True)
        b = torch.randn((E,) if h == 1 else (E, h), generator=gen, device=dev).requires_grad_(True)
        dO = torch.randn(ns(n_q), generator=gen, device=dev) / d ** 0.5
        leaves = (Q, K, V, xe, b)

        def clear():
            for x in leaves:
                x.grad = None

        for p in (float(x) for x in args.dropout.split(",")):
            drop = (p, args.dropout_seed, 7)

            def edge():
                clear()
                return functions.fused_attention_edge_step(g, Q, K, V, xe, dO, *drop)

            def no_edge():
                clear()
                return functions.fused_attention_bias_step(g, Q, K, V, b, dO, *drop)

            def composed():
                clear()
                return functions.attention_edge_step(g, Q, K, V, xe, dO, *drop)

            fns = {"edge": edge, "no_edge": no_edge}
            err, composed_note = None, "left out (--no-composed)"
            if not args.no_composed:
                try:      # full-size comparison
                    o_c = composed()[2].detach()
                    want = [o_c] + [x.grad.clone() for x in leaves[:4]]
                    o_f = edge().detach()
                    got = [o_f] + [x.grad.clone() for x in leaves[:4]]
                    torch.cuda.synchronize()
                    err = {n: _node_err(x, y) for n, x, y in zip(("o", "dQ", "dK", "dV"), got, want)}
                    err["dxe"] = float((got[4] - want[4]).abs().max() / want[4].abs().max())
                    del o_c, o_f, want, got
                    fns["composed"] = composed
                    composed_note = "ran"
                except torch.OutOfMemoryError:
                    composed_note = "out of memory"
                clear()
                torch.cuda.empty_cache()
            peak = {}
            for name, fn in fns.items():
                fn()      # plans, caches
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
            timings = {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                           "max_ms": round(max(v), 4)} for n, v in t.items()}
            prof, prof0 = _profile(edge, args.iters), _profile(no_edge, args.iters)
            F = h * d
            rows = 4 * E * F                                          # one (E, h, d) stream: a row gather, xe or dxe
            ids_r, ids_c = 8 * E + 16 * C_r, 8 * E + 16 * C_c
            eid_r = 0 if identity else 8 * E
            node_q, node_k, st = 4 * n_q * F, 4 * n_k * F, 8 * n_q * h
            model = {   # tag: (node tables and ids, row gathers per slot, edge-stream bytes)
                "attn_edge_fwd_rows": (ids_r + 2 * node_q + st, 2, rows + eid_r),
                "attn_edge_rows_row": (ids_r + 3 * node_q + 2 * st, 2, 2 * rows + eid_r),
                "attn_edge_rows_col": (ids_c + 4 * node_k, 2, rows + 8 * E),
            }
            kernels = {}
            for tag, q in sorted(prof.items()):
                if not tag.startswith("attn_edge"):
                    continue
                rec = {"kernel": q["kernel"], "calls": q["calls"], "mean_ms": round(q["mean_ms"], 4), "min_ms": round(q["min_ms"], 4)}
                if tag in model:
                    nbytes, gathers, edge_bytes = model[tag]
                    sec = q["mean_ms"] * 1e-3
                    rec.update(node_and_id_bytes=nbytes, gathered_row_bytes=gathers * rows, edge_stream_bytes=edge_bytes,
                               edge_stream_fraction_of_8TBs=round(edge_bytes / sec / PEAK, 3),
                               all_bytes_fraction_of_8TBs=round((nbytes + gathers * rows + edge_bytes) / sec / PEAK, 3))
                kernels[tag] = rec
            kernels_no_edge = {tag: {"kernel": q["kernel"], "calls": q["calls"], "mean_ms": round(q["mean_ms"], 4)}
                               for tag, q in sorted(prof0.items()) if tag.startswith("attn_")}
            f = timings["edge"]["median_ms"]
            rec = {
                "tool": "tools/time_fused_attention_edge.py",
                "graph": "chung_lu_graph(%d, %d, alpha=0.5, seed=%d)" % (N, E, args.seed), "shape": args.shape,
                "n_q": n_q, "n_k": n_k, "n_edges": E, "row_chunks": C_r, "col_chunks": C_c, "chunk_size": args.chunk_size,
                "h": h, "d": d, "dropout": {"p": drop[0], "seed": drop[1], "offset": drop[2]}, "eid_identity": identity,
                "knobs": {"attn_heads": 1, "attn_rows": 1}, "warmup": args.warmup, "iters": args.iters,
                "composed": composed_note, "node_scaled_difference_vs_composed": err, "timings": timings,
                "edge_over_no_edge": round(f / timings["no_edge"]["median_ms"], 3),
                "edge_over_composed": round(f / timings["composed"]["median_ms"], 3) if "composed" in timings else None,
                "peak_added_bytes": peak, "one_edge_row_tensor_bytes": rows, "kernels": kernels,
                "kernels_no_edge": kernels_no_edge, "device": torch.cuda.get_device_name(dev)}
            print(json.dumps(rec), flush=True)
            records.append(rec)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:      # rewritten after every case: a run that is cut short keeps what it has
                json.dump(records, fh, indent=1)
                fh.write("\n")
        del Q, K, V, xe, b, dO, leaves
        torch.cuda.empty_cache()
    _lib.check_errors()


if __name__ == "__main__":
    main()
