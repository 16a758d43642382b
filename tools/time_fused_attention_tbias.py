#!/usr/bin/env python3
"""Time the fused dot-product attention step with an edge-type score bias (functions.fused_attention_tbias_step:
FusedAttentionTypeBias, one autograd node, nothing edge-sized but the int32 types).

Three steps alternate in one process, --warmup untimed rounds and then --iters rounds timed by device events:
  tbias     the fused typed step;
  gather    what a user runs without it: functions.fused_attention_bias_step on b = B[etype] under autograd, whose
            backward index_adds the (E, h) gradient db into B.grad (the gather and the index_add are inside the timed
            step);
  stream    functions.fused_attention_bias_step on a fixed b = B[etype] that takes no gradient: the same chunk-driver
            family with a per-edge stream in place of the table, and no db store.
All three run under the knobs attn_heads = 1 and attn_rows = 1, which put the per-edge bias op on the several-head
chunk-driver kernels.  Reported per (h, d), p and n_types: medians (min..max), the peak memory each step adds to what is
allocated before it, the per-pass kernel times of the library's launch profile (rounds of their own) for each step next
to the bytes of the model of 4.5p -- per pass those of 4.5l with 4 E of etype in place of 4 E h of b, 8 E of eid unless
the row-major plan says identity (the column pass always pays it, and its type is a random 4-byte read per slot), the
table from cache and no db store -- and the largest node-scaled error of the typed step against the gather step (dB by
the tensor's largest value).  Nothing is asserted on a time.
Graph: chung_lu_graph(N of --shape, --edges or the shape's E, alpha=0.5, seed=--seed).  One JSON record per case, printed
and collected in --out (default profiles/fused_attention_tbias_bench.json; --append keeps the records already there)."""
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
    ap.add_argument("--edges", type=int, default=20_000_000, metavar="N", help="N edges instead of the default 20 M")
    ap.add_argument("--hd", default="1x64,8x8,8x32", help="comma-separated h x d pairs")
    ap.add_argument("--dropout", default="0,0.3", help="comma-separated dropout probabilities")
    ap.add_argument("--types", default="4,64", help="comma-separated numbers of edge types")
    ap.add_argument("--dropout-seed", type=int, default=1234567890123)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk-size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--append", action="store_true", help="keep the records --out already holds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_attention_tbias_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, _ = graphs.SHAPES[args.shape]
    g = graphs.chung_lu_graph(N, args.edges, alpha=0.5, seed=args.seed, chunk_size=args.chunk_size, device=dev)
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
        dO = torch.randn(ns(n_q), generator=gen, device=dev) / d ** 0.5
        for n_types in (int(x) for x in args.types.split(",")):
            B = torch.randn((n_types,) if h == 1 else (n_types, h), generator=gen, device=dev).requires_grad_(True)
            etype = torch.randint(0, n_types, (E,), generator=gen, device=dev).to(torch.int32)
            etype_long = etype.long()          # the gather's index, made once: not part of the user's step
            b_fixed = B.detach().index_select(0, etype_long).contiguous()
            leaves = (Q, K, V, B)

            def clear():
                for x in leaves:
                    x.grad = None

            for p in (float(x) for x in args.dropout.split(",")):
                drop = (p, args.dropout_seed, 7)

                def tbias():
                    clear()
                    return functions.fused_attention_tbias_step(g, Q, K, V, B, etype, dO, *drop)

                def gather():
                    clear()
                    return functions.fused_attention_bias_step(g, Q, K, V, B.index_select(0, etype_long), dO, *drop)

                def stream():
                    clear()
                    return functions.fused_attention_bias_step(g, Q, K, V, b_fixed, dO, *drop)

                fns = {"tbias": tbias, "gather": gather, "stream": stream}
                o_g = gather().detach()
                want = [o_g] + [x.grad.clone() for x in leaves]
                o_t = tbias().detach()
                got = [o_t] + [x.grad.clone() for x in leaves]
                torch.cuda.synchronize()
                err = {n: _node_err(x, y) for n, x, y in zip(("o", "dQ", "dK", "dV"), got, want)}
                err["dB"] = float((got[4] - want[4]).abs().max() / want[4].abs().max())
                del o_g, o_t, want, got
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
                prof, prof_g, prof_s = (_profile(fn, args.iters) for fn in (tbias, gather, stream))
                F = h * d
                rows = 4 * E * F                                          # one (E, h, d) stream: a row gather
                ids_r, ids_c = 8 * E + 16 * C_r, 8 * E + 16 * C_c
                eid_r = 0 if identity else 8 * E
                node_q, node_k, st = 4 * n_q * F, 4 * n_k * F, 8 * n_q * h
                model = {   # tag: (node tables and ids, row gathers per slot, edge-stream bytes: etype and eid)
                    "attn_tbias_fwd_rows": (ids_r + 2 * node_q + st, 2, 4 * E + eid_r),
                    "attn_tbias_rows_row": (ids_r + 3 * node_q + 2 * st, 2, 4 * E + eid_r),
                    "attn_tbias_rows_col": (ids_c + 4 * node_k, 2, 4 * E + 8 * E),
                }
                kernels = {}
                for tag, q in sorted(prof.items()):
                    if not tag.startswith("attn_tbias"):
                        continue
                    rec = {"kernel": q["kernel"], "calls": q["calls"], "mean_ms": round(q["mean_ms"], 4), "min_ms": round(q["min_ms"], 4)}
                    if tag in model:
                        nbytes, gathers, edge_bytes = model[tag]
                        sec = q["mean_ms"] * 1e-3
                        rec.update(node_and_id_bytes=nbytes, gathered_row_bytes=gathers * rows, edge_stream_bytes=edge_bytes,
                                   all_bytes_fraction_of_8TBs=round((nbytes + gathers * rows + edge_bytes) / sec / PEAK, 3))
                    kernels[tag] = rec
                others = [{tag: {"kernel": q["kernel"], "calls": q["calls"], "mean_ms": round(q["mean_ms"], 4)}
                           for tag, q in sorted(pr.items()) if tag.startswith("attn_")} for pr in (prof_g, prof_s)]
                f = timings["tbias"]["median_ms"]
                rec = {
                    "tool": "tools/time_fused_attention_tbias.py",
                    "graph": "chung_lu_graph(%d, %d, alpha=0.5, seed=%d)" % (N, E, args.seed), "shape": args.shape,
                    "n_q": n_q, "n_k": n_k, "n_edges": E, "row_chunks": C_r, "col_chunks": C_c, "chunk_size": args.chunk_size,
                    "h": h, "d": d, "n_types": n_types, "dropout": {"p": drop[0], "seed": drop[1], "offset": drop[2]},
                    "eid_identity": identity, "knobs": {"attn_heads": 1, "attn_rows": 1}, "warmup": args.warmup,
                    "iters": args.iters, "node_scaled_difference_vs_gather_step": err, "timings": timings,
                    "tbias_over_gather": round(f / timings["gather"]["median_ms"], 3),
                    "tbias_over_stream": round(f / timings["stream"]["median_ms"], 3),
                    "peak_added_bytes": peak, "one_edge_bias_tensor_bytes": 4 * E * h, "kernels": kernels,
                    "kernels_gather": others[0], "kernels_stream": others[1], "device": torch.cuda.get_device_name(dev)}
                print(json.dumps(rec), flush=True)
                records.append(rec)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as fh:      # rewritten after every case: a run that is cut short keeps what it has
                    json.dump(records, fh, indent=1)
                    fh.write("\n")
            del B, etype, etype_long, b_fixed, leaves
        del Q, K, V, dO
        torch.cuda.empty_cache()
    _lib.check_errors()


if __name__ == "__main__":
    main()
