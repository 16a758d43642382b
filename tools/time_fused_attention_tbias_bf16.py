#!/usr/bin/env python3
"""Time the bfloat16 fused attention step with an edge-type score bias (functions.fused_attention_tbias_step on bfloat16
leaves: FusedAttentionTypeBias over graphop.attention_tbias_bf16_*).

Four steps alternate in one process, --warmup untimed rounds and then --iters rounds timed by device events:
  tbias     (a) the fused typed step on bfloat16 tables;
  gather    (b) what a bfloat16 user ran without it: functions.fused_attention_bias_step on b = B[etype] under autograd,
            whose backward index_adds the (E, h) bfloat16 db into B.grad (gather and index_add inside the timed step);
  stream    (c) functions.fused_attention_bias_step on a fixed bfloat16 b = B[etype] that takes no gradient: the same
            kernels with a per-edge stream in place of the LDS table, and no db store;
  fp32      (d) the fp32 FusedAttentionTypeBias of 4.5p on the same values widened, under attn_heads = attn_rows = 1.
A step whose first call takes longer than --slow-ms (the gather step: torch's bfloat16 index_add onto a few rows takes
seconds) stays out of the rounds and is reported by that one call's wall-clock time.
Reported per (h, d), p and n_types: medians (min..max), the per-pass kernel times of the library's launch profile for
the typed step (rounds of their own), the largest node-scaled difference of o, dQ, dK, dV against the stream step, and
B.grad of the typed and of the gather step against the fp32 step's.  Nothing is asserted on a time.
Graph: chung_lu_graph(N of --shape, --edges (20 M, as tools/time_fused_attention_tbias.py), alpha=0.5, seed=--seed).  One JSON record per case, printed
and collected in --out (default profiles/fused_attention_tbias_bf16_bench.json; --append keeps the records there)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from custom_op_benchmark_amd import _lib, functions, graphs  # noqa: E402
from time_fused_attention_edge import _node_err, _profile, _timed  # noqa: E402


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
    ap.add_argument("--slow-ms", type=float, default=1000.0, help="a step slower than this is timed by its one first call")
    ap.add_argument("--chunk-size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--append", action="store_true", help="keep the records --out already holds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_attention_tbias_bf16_bench.json"))
    args = ap.parse_args()
    dev, bf = torch.device("cuda:0"), torch.bfloat16
    N, _ = graphs.SHAPES[args.shape]
    g = graphs.chung_lu_graph(N, args.edges, alpha=0.5, seed=args.seed, chunk_size=args.chunk_size, device=dev)
    E, n_q, n_k = g.n_edges, g.n_src, g.n_dst
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
        Q = (torch.randn(ns(n_q), generator=gen, device=dev) / d ** 0.5).to(bf).requires_grad_(True)
        K = torch.randn(ns(n_k), generator=gen, device=dev).to(bf).requires_grad_(True)
        V = torch.randn(ns(n_k), generator=gen, device=dev).to(bf).requires_grad_(True)
        dO = (torch.randn(ns(n_q), generator=gen, device=dev) / d ** 0.5).to(bf)
        Qf, Kf, Vf = (x.detach().float().requires_grad_(True) for x in (Q, K, V))
        dOf = dO.float()
        for n_types in (int(x) for x in args.types.split(",")):
            B = torch.randn((n_types,) if h == 1 else (n_types, h), generator=gen, device=dev).to(bf).requires_grad_(True)
            Bf = B.detach().float().requires_grad_(True)
            etype = torch.randint(0, n_types, (E,), generator=gen, device=dev).to(torch.int32)
            etype_long = etype.long()          # the gather's index, made once: not part of the user's step
            b_fixed = B.detach().index_select(0, etype_long).contiguous()
            leaves = (Q, K, V, B, Qf, Kf, Vf, Bf)

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

                def fp32():
                    clear()
                    return functions.fused_attention_tbias_step(g, Qf, Kf, Vf, Bf, etype, dOf, *drop)

                fns = {"tbias": tbias, "gather": gather, "stream": stream, "fp32": fp32}
                first, grads = {}, {}
                for name, fn in fns.items():          # plans and caches; how long one call takes, said at once
                    t0 = time.perf_counter()
                    o = fn().detach()
                    torch.cuda.synchronize()
                    first[name] = 1e3 * (time.perf_counter() - t0)
                    grads[name] = [o] + [None if x.grad is None else x.grad.clone()          # (stream: no B.grad)
                                         for x in (leaves[4:] if name == "fp32" else leaves[:4])]
                    print("%dx%d T=%d p=%g first %s: %.1f ms" % (h, d, n_types, p, name, first[name]), file=sys.stderr, flush=True)
                # o, dQ, dK, dV against the per-edge step; the table's gradient against the fp32 step's, since the gather
                # step's index_add sums B.grad in bfloat16
                err = {n: _node_err(x, y) for n, x, y in zip(("o", "dQ", "dK", "dV"), grads["tbias"], grads["stream"])}
                dB32 = grads["fp32"][4].double()
                err["dB_vs_fp32"] = float((grads["tbias"][4].double() - dB32).abs().max() / dB32.abs().max())
                err["gather_dB_vs_fp32"] = float((grads["gather"][4].double() - dB32).abs().max() / dB32.abs().max())
                del grads, o, dB32
                # a step whose one call takes more than --slow-ms is not put through the rounds: its time is that call's
                slow = {n for n, ms in first.items() if ms > args.slow_ms}
                t = _timed({n: fn for n, fn in fns.items() if n not in slow}, args.warmup, args.iters)
                timings = {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                               "max_ms": round(max(v), 4)} for n, v in t.items()}
                timings.update({n: {"median_ms": round(first[n], 1), "min_ms": round(first[n], 1), "max_ms": round(first[n], 1),
                                    "one_call_wall_clock": True} for n in slow})
                kernels = {tag: {"kernel": q["kernel"], "calls": q["calls"], "mean_ms": round(q["mean_ms"], 4),
                                 "min_ms": round(q["min_ms"], 4)}
                           for tag, q in sorted(_profile(tbias, args.iters).items()) if tag.startswith("attn_tbias_bf16")}
                a = timings["tbias"]["median_ms"]
                rec = {"tool": "tools/time_fused_attention_tbias_bf16.py",
                       "graph": "chung_lu_graph(%d, %d, alpha=0.5, seed=%d)" % (N, E, args.seed), "shape": args.shape,
                       "n_q": n_q, "n_k": n_k, "n_edges": E, "row_chunks": g.n_row_chunks, "col_chunks": g.n_col_chunks,
                       "chunk_size": args.chunk_size, "h": h, "d": d, "n_types": n_types,
                       "dropout": {"p": drop[0], "seed": drop[1], "offset": drop[2]},
                       "knobs": {"attn_heads": 1, "attn_rows": 1}, "warmup": args.warmup, "iters": args.iters,
                       "node_scaled_difference_vs_stream_step": err, "timings": timings,
                       "tbias_over_gather": round(a / timings["gather"]["median_ms"], 3),
                       "tbias_over_stream": round(a / timings["stream"]["median_ms"], 3),
                       "tbias_over_fp32": round(a / timings["fp32"]["median_ms"], 3), "kernels": kernels,
                       "device": torch.cuda.get_device_name(dev)}
                print(json.dumps(rec), flush=True)
                records.append(rec)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as fh:      # rewritten after every case: a run that is cut short keeps what it has
                    json.dump(records, fh, indent=1)
                    fh.write("\n")
            del B, Bf, etype, etype_long, b_fixed, leaves
        del Q, K, V, dO, Qf, Kf, Vf, dOf
        torch.cuda.empty_cache()
    _lib.check_errors()


if __name__ == "__main__":
    main()
