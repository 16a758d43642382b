#!/usr/bin/env python3
"""Time the bfloat16 fused attention step with edge-type embeddings (functions.fused_attention_etype_step on bfloat16
leaves: FusedAttentionEdgeType over graphop.attention_etype_bf16_*).

Four steps alternate in one process, --warmup untimed rounds and then --iters rounds timed by device events:
  typed     (a) the fused typed step on bfloat16 tables;
  gather    (b) what a bfloat16 user ran without it: functions.fused_attention_edge_step on xe = R[etype] under autograd
            (gather inside the timed step); where R takes a gradient the backward stores the (E, h, d) bfloat16 dxe and
            index_adds it into R.grad;
  fp32      (c) the fp32 FusedAttentionEdgeType of 4.5o on the same values widened, under attn_heads = attn_rows = 1;
  plain     (d) functions.fused_attention_dropout_step on the same bfloat16 Q, K, V: the step without any edge term.
Every case runs with and without R.grad.  A step whose first call takes longer than --slow-ms (the gather step with
R.grad: torch's bfloat16 index_add onto a few rows takes seconds) stays out of the rounds and is reported by that one
call's wall-clock time.  Reported per (h, d), p, n_types and R.grad: medians only, the per-pass kernel times of the
library's launch profile for the typed step (rounds of their own), and, with --quality (small graphs: the float64 op runs
generic kernels), the largest error of R.grad of the typed and of the gather step against the float64 typed step, in
units of the largest |R.grad|.  Nothing is asserted on a time.
Graph: chung_lu_graph(N of --shape, --edges, alpha=0.5, seed=--seed).  One JSON record per case, printed and collected in
--out (default profiles/fused_attention_etype_bf16_bench.json; --append keeps the records there)."""
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
from time_fused_attention_edge import _profile, _timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", default="reddit", choices=sorted(graphs.SHAPES))
    ap.add_argument("--edges", type=int, default=20_000_000, metavar="N", help="N edges instead of the default 20 M")
    ap.add_argument("--hd", default="1x64,4x64,8x32", help="comma-separated h x d pairs")
    ap.add_argument("--dropout", default="0", help="comma-separated dropout probabilities")
    ap.add_argument("--types", default="16", help="comma-separated numbers of edge types")
    ap.add_argument("--dropout-seed", type=int, default=1234567890123)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--slow-ms", type=float, default=1000.0, help="a step slower than this is timed by its one first call")
    ap.add_argument("--quality", action="store_true", help="R.grad of the typed and the gather step against float64")
    ap.add_argument("--chunk-size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--append", action="store_true", help="keep the records --out already holds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_attention_etype_bf16_bench.json"))
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
            R = torch.randn(ns(n_types), generator=gen, device=dev).to(bf)
            Rf = R.float()
            etype = torch.randint(0, n_types, (E,), generator=gen, device=dev).to(torch.int32)
            etype_long = etype.long()          # the gather's index, made once: not part of the user's step
            n_max = int(torch.bincount(etype_long).max())
            leaves = (Q, K, V, R, Qf, Kf, Vf, Rf)
            for p in (float(x) for x in args.dropout.split(",")):
                drop = (p, args.dropout_seed, 7)
                quality = None
                for r_grad in (True, False):
                    R.requires_grad_(r_grad)
                    Rf.requires_grad_(r_grad)

                    def clear():
                        for x in leaves:
                            x.grad = None

                    def typed():
                        clear()
                        return functions.fused_attention_etype_step(g, Q, K, V, R, etype, dO, *drop)

                    def gather():
                        clear()
                        return functions.fused_attention_edge_step(g, Q, K, V, R.index_select(0, etype_long), dO, *drop)

                    def fp32():
                        clear()
                        return functions.fused_attention_etype_step(g, Qf, Kf, Vf, Rf, etype, dOf, *drop)

                    def plain():
                        clear()
                        return functions.fused_attention_dropout_step(g, Q, K, V, dO, *drop)

                    fns = {"typed": typed, "gather": gather, "fp32": fp32, "plain": plain}
                    first, rgrad = {}, {}
                    for name, fn in fns.items():          # plans and caches; how long one call takes, said at once
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        first[name] = 1e3 * (time.perf_counter() - t0)
                        if r_grad and name in ("typed", "gather"):
                            rgrad[name] = R.grad.double()
                        print("%dx%d T=%d p=%g R.grad=%s first %s: %.1f ms" % (h, d, n_types, p, r_grad, name, first[name]),
                              file=sys.stderr, flush=True)
                    if r_grad and args.quality:          # the float64 typed step: the library's own op on widened leaves
                        Q64, K64, V64, R64 = (x.detach().double().requires_grad_(True) for x in (Q, K, V, R))
                        functions.fused_attention_etype_step(g, Q64, K64, V64, R64, etype, dO.double(), *drop)
                        ref = R64.grad
                        quality = {"n_max": n_max, "largest_abs_R_grad": float(ref.abs().max()),
                                   "typed_max_err_over_largest": float((rgrad["typed"] - ref).abs().max() / ref.abs().max()),
                                   "gather_max_err_over_largest": float((rgrad["gather"] - ref).abs().max() / ref.abs().max())}
                        del Q64, K64, V64, R64, ref
                    del rgrad
                    slow = {n for n, ms in first.items() if ms > args.slow_ms}
                    t = _timed({n: fn for n, fn in fns.items() if n not in slow}, args.warmup, args.iters)
                    medians = {n: round(statistics.median(v), 4) for n, v in t.items()}
                    medians.update({n: round(first[n], 1) for n in slow})
                    kernels = {tag: round(q["mean_ms"], 4) for tag, q in sorted(_profile(typed, args.iters).items())
                               if tag.startswith("attn_etype_bf16")}
                    a = medians["typed"]
                    rec = {"tool": "tools/time_fused_attention_etype_bf16.py", "shape": args.shape, "n_q": n_q, "n_k": n_k,
                           "n_edges": E, "h": h, "d": d, "n_types": n_types, "n_max": n_max, "p": p, "R_grad": r_grad,
                           "warmup": args.warmup, "iters": args.iters, "median_ms": medians,
                           "one_call_wall_clock": sorted(slow), "typed_over_gather": round(a / medians["gather"], 3),
                           "typed_over_fp32": round(a / medians["fp32"], 3), "typed_over_plain": round(a / medians["plain"], 3),
                           "typed_kernels_mean_ms": kernels, "device": torch.cuda.get_device_name(dev)}
                    if quality and r_grad:
                        rec["R_grad_quality_vs_float64"] = quality
                    print(json.dumps(rec), flush=True)
                    records.append(rec)
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "w") as fh:      # rewritten after every case: a run that is cut short keeps what it has
                        fh.write("[\n" + ",\n".join(json.dumps(r) for r in records) + "\n]\n")          # a record a line
            del R, Rf, etype, etype_long, leaves
        del Q, K, V, dO, Qf, Kf, Vf, dOf
        torch.cuda.empty_cache()
    _lib.check_errors()


if __name__ == "__main__":
    main()
