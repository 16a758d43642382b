#!/usr/bin/env python3
"""Time the fused dot-product attention step with edge-type embeddings (functions.fused_attention_etype_step:
FusedAttentionEdgeType, one autograd node, nothing edge-sized but the int32 types).

Three steps alternate in one process, --warmup untimed rounds and then --iters rounds timed by device events:
  etype     the fused typed step;
  edge      what a user runs without it: functions.fused_attention_edge_step on a materialised xe = R[etype] under
            autograd, whose backward index_adds the (E, h, d) gradient into R.grad (the gather is inside the timed step);
  no_edge   functions.fused_attention_bias_step with the knobs attn_heads = 1 and attn_rows = 1: the same chunk-driver
            family without an edge term (its edge-sized operands are the (E, h) bias and its gradient).
Reported per (h, d), p and n_types: medians (min..max), the peak memory each step adds to what is allocated before it,
the per-pass kernel times of the library's launch profile (rounds of their own) for the typed step and for the edge step
next to the bytes of the model of 4.5o -- per pass those of 4.5l plus 4 E of etype, 8 E of eid unless the row-major plan
says identity (the column pass always pays it, and its type is a random 4-byte read per slot) and the table from cache --
and the largest node-scaled error of the typed step against the edge step (dR by the tensor's largest value).  Nothing
is asserted on a time.
Graph: chung_lu_graph(N of --shape, --edges or the shape's E, alpha=0.5, seed=--seed).  One JSON record per case, printed
and collected in --out (default profiles/fused_attention_etype_bench.json; --append keeps the records already there)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from custom_op_benchmark_amd import _lib, functions, graphs  # noqa: E402
from time_fused_attention_edge import PEAK, _node_err, _profile, _timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", default="reddit", choices=sorted(graphs.SHAPES))
    ap.add_argument("--edges", type=int, default=None, metavar="N", help="N edges instead of the shape's")
    ap.add_argument("--hd", default="1x64,8x8,8x32", help="comma-separated h x d pairs")
    ap.add_argument("--dropout", default="0,0.3", help="comma-separated dropout probabilities")
    ap.add_argument("--types", default="4,16", help="comma-separated numbers of edge types")
    ap.add_argument("--dropout-seed", type=int, default=1234567890123)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk-size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--append", action="store_true", help="keep the records --out already holds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_attention_etype_bench.json"))
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
        b = torch.randn((E,) if h == 1 else (E, h), generator=gen, device=dev).requires_grad_(True)
        dO = torch.randn(ns(n_q), generator=gen, device=dev) / d ** 0.5
        for n_types in (int(x) for x in args.types.split(",")):
            R = torch.randn(ns(n_types), generator=gen, device=dev).requires_grad_(True)
            etype = torch.randint(0, n_types, (E,), generator=gen, device=dev).to(torch.int32)
            etype_long = etype.long()          # the gather's index, made once: not part of the user's step
            leaves = (Q, K, V, R, b)

            def clear():
                for x in leaves:
                    x.grad = None

            for p in (float(x) for x in args.dropout.split(",")):
                drop = (p, args.dropout_seed, 7)

                def typed():
                    clear()
                    return functions.fused_attention_etype_step(g, Q, K, V, R, etype, dO, *drop)

                def edge():
                    clear()
                    return functions.fused_attention_edge_step(g, Q, K, V, R.index_select(0, etype_long), dO, *drop)

                def no_edge():
                    clear()
                    return functions.fused_attention_bias_step(g, Q, K, V, b, dO, *drop)

                fns = {"etype": typed, "edge": edge, "no_edge": no_edge}
                o_e = edge().detach()
                want = [o_e] + [x.grad.clone() for x in leaves[:4]]
                o_t = typed().detach()
                got = [o_t] + [x.grad.clone() for x in leaves[:4]]
                torch.cuda.synchronize()
                err = {n: _node_err(x, y) for n, x, y in zip(("o", "dQ", "dK", "dV"), got, want)}
                err["dR"] = float((got[4] - want[4]).abs().max() / want[4].abs().max())
                del o_e, o_t, want, got
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
                prof, prof_e, prof0 = (_profile(fn, args.iters) for fn in (typed, edge, no_edge))
                F = h * d
                rows = 4 * E * F                                          # one (E, h, d) stream: a row gather
                ids_r, ids_c = 8 * E + 16 * C_r, 8 * E + 16 * C_c
                eid_r = 0 if identity else 8 * E
                node_q, node_k, st = 4 * n_q * F, 4 * n_k * F, 8 * n_q * h
                model = {   # tag: (node tables and ids, row gathers per slot, edge-stream bytes: etype and eid)
                    "attn_etype_fwd_rows": (ids_r + 2 * node_q + st, 2, 4 * E + eid_r),
                    "attn_etype_rows_row": (ids_r + 3 * node_q + 2 * st, 2, 4 * E + eid_r),
                    "attn_etype_rows_col": (ids_c + 4 * node_k, 2, 4 * E + 8 * E),
                }
                kernels = {}
                for tag, q in sorted(prof.items()):
                    if not tag.startswith("attn_etype"):
                        continue
                    rec = {"kernel": q["kernel"], "calls": q["calls"], "mean_ms": round(q["mean_ms"], 4), "min_ms": round(q["min_ms"], 4)}
                    if tag in model:
                        nbytes, gathers, edge_bytes = model[tag]
                        sec = q["mean_ms"] * 1e-3
                        rec.update(node_and_id_bytes=nbytes, gathered_row_bytes=gathers * rows, edge_stream_bytes=edge_bytes,
                                   all_bytes_fraction_of_8TBs=round((nbytes + gathers * rows + edge_bytes) / sec / PEAK, 3))
                    kernels[tag] = rec
                others = [{tag: {"kernel": q["kernel"], "calls": q["calls"], "mean_ms": round(q["mean_ms"], 4)}
                           for tag, q in sorted(pr.items()) if tag.startswith("attn_")} for pr in (prof_e, prof0)]
                f = timings["etype"]["median_ms"]
                rec = {
                    "tool": "tools/time_fused_attention_etype.py",
                    "graph": "chung_lu_graph(%d, %d, alpha=0.5, seed=%d)" % (N, E, args.seed), "shape": args.shape,
                    "n_q": n_q, "n_k": n_k, "n_edges": E, "row_chunks": C_r, "col_chunks": C_c, "chunk_size": args.chunk_size,
                    "h": h, "d": d, "n_types": n_types, "dropout": {"p": drop[0], "seed": drop[1], "offset": drop[2]},
                    "eid_identity": identity, "knobs": {"attn_heads": 1, "attn_rows": 1}, "warmup": args.warmup,
                    "iters": args.iters, "node_scaled_difference_vs_edge_step": err, "timings": timings,
                    "etype_over_edge": round(f / timings["edge"]["median_ms"], 3),
                    "etype_over_no_edge": round(f / timings["no_edge"]["median_ms"], 3),
                    "peak_added_bytes": peak, "one_edge_row_tensor_bytes": rows, "kernels": kernels,
                    "kernels_edge": others[0], "kernels_no_edge": others[1], "device": torch.cuda.get_device_name(dev)}
                print(json.dumps(rec), flush=True)
                records.append(rec)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as fh:      # rewritten after every case: a run that is cut short keeps what it has
                    json.dump(records, fh, indent=1)
                    fh.write("\n")
            del R, etype, etype_long, leaves
        del Q, K, V, b, dO
        torch.cuda.empty_cache()
    _lib.check_errors()


if __name__ == "__main__":
    main()
