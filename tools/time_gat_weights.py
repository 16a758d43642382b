#!/usr/bin/env python3
"""Time graphop.gat_attention_weights / gatv2_attention_weights (the weights of the fused GAT and GATv2 layers from their
row statistics) against the routes a user had before them.

Per form and shape, candidates alternate in one process, --warmup untimed rounds and then --iters rounds timed by device
events:
  gat, gatv2            weights   the new op on the statistics of the matching fused forward
                        composed  sparse_softmax_forward(gat_scores_forward / gatv2_scores_forward): a second softmax
                        forward   the matching fused forward (its own launch profile is recorded too)
  gat_edge, gatv2_edge  weights   the new op with ee / xe
                        composed  the forward of gat_edge_attention_step / gatv2_edge_attention_step up to a (GATScores at
                                  slope 1 + torch arithmetic; torch gathers of (E, h, d) rows), on the graph cut to
                                  --edge-edges for gatv2_edge, where those temporaries fit
                        forward   the matching fused forward
Reported: medians (min..max), the peak memory each candidate adds to what is allocated before it, the per-kernel times
of the library's launch profile, and the largest relative difference between the candidates' weights.  Nothing is
asserted on a time.  Graph: chung_lu_graph(232965, --edges, alpha=0.5, seed=--seed), identity edge ids, fp32.  One JSON
record per case, printed and collected in --out (default profiles/gat_attention_weights_bench.json)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from custom_op_benchmark_amd import _lib, graphs, graphop as ops  # noqa: E402


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


def _profile(fn, iters):
    _lib.profile_enable(True)
    try:
        _lib.profile_read()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        prof = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    return {t: {"kernel": q["kernel"], "calls": q["calls"], "mean_ms": round(q["mean_ms"], 4), "min_ms": round(q["min_ms"], 4)}
            for t, q in sorted(prof.items())}


def _peaks(fns):
    peak = {}
    for name, fn in fns.items():
        fn()      # plans, caches
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
        del out
    return peak


def _summary(t):
    return {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for n, v in t.items()}


def _rel(x, y):
    return float(((x - y).abs() / y.abs().clamp_min(1e-30)).max())


def _case(form, g, h, d, seed, dev, slope=0.2):
    """-> {candidate: fn} of one form on graph g"""
    gen = torch.Generator(device=dev).manual_seed(seed + h * 100 + d)
    a4 = g.csr_args()[:4]
    a3 = a4[:3]
    edge = form.endswith("_edge")
    if form.startswith("gatv2"):
        ns = (lambda n: (n, d) if h == 1 else (n, h, d))
        xl, xr = torch.randn(ns(g.n_src), generator=gen, device=dev), torch.randn(ns(g.n_dst), generator=gen, device=dev)
        att = torch.randn(ns(1)[1:], generator=gen, device=dev) / d ** 0.5
        xe = torch.randn(ns(g.n_edges), generator=gen, device=dev) if edge else None
        forward = lambda: ops.gatv2_attention_dropout_forward(*a4, xl, xr, att, slope, xe=xe)  # noqa: E731
        stats = forward()[1]
        weights = lambda: ops.gatv2_attention_weights(*a4, xl, xr, att, stats, xe, slope)  # noqa: E731
        if edge:
            # g.src / g.dst are in edge-id order, eid_r in slot order: one order only with identity edge ids
            assert torch.equal(g.eid_r, torch.arange(g.n_edges, device=dev))

            def composed():
                z = (xl.index_select(0, g.src) + xr.index_select(0, g.dst)) + xe.index_select(0, g.eid_r)
                s_slot = (F.leaky_relu(z, slope) * att).sum(-1)
                s = torch.zeros_like(s_slot).index_copy(0, g.eid_r, s_slot)
                return ops.sparse_softmax_forward(*a3, s)
        else:
            composed = lambda: ops.sparse_softmax_forward(*a3, ops.gatv2_scores_forward(*a4, xl, xr, att, slope))  # noqa: E731
    else:
        ns = (lambda n: (n,) if h == 1 else (n, h))
        el, er = torch.randn(ns(g.n_src), generator=gen, device=dev), torch.randn(ns(g.n_dst), generator=gen, device=dev)
        V = torch.randn((g.n_dst, d) if h == 1 else (g.n_dst, h, d), generator=gen, device=dev)
        ee = torch.randn(ns(g.n_edges), generator=gen, device=dev) if edge else None
        if edge:
            forward = lambda: ops.gat_edge_attention_forward(*a4, el, er, ee, V, slope)  # noqa: E731
            composed = lambda: ops.sparse_softmax_forward(  # noqa: E731
                *a3, F.leaky_relu(ops.gat_scores_forward(*a4, el, er, 1.0) + ee, slope))
        else:
            forward = lambda: ops.gat_attention_forward(*a4, el, er, V, slope)  # noqa: E731
            composed = lambda: ops.sparse_softmax_forward(*a3, ops.gat_scores_forward(*a4, el, er, slope))  # noqa: E731
        stats = forward()[1]
        weights = lambda: ops.gat_attention_weights(*a4, el, er, stats, ee, slope)  # noqa: E731
    return {"weights": weights, "composed": composed, "forward": forward}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--edge-edges", type=int, default=2_000_000, help="edges of the cut graph of the gatv2_edge form")
    ap.add_argument("--hd", default="1x64,4x16,8x8,8x32", help="comma-separated h x d pairs")
    ap.add_argument("--forms", default="gat,gat_edge,gatv2,gatv2_edge")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk-size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gat_attention_weights_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    graph_of = {}

    def graph(E):
        if E not in graph_of:
            graph_of[E] = graphs.chung_lu_graph(args.nodes, E, alpha=0.5, seed=args.seed, chunk_size=args.chunk_size,
                                                device=dev)
        return graph_of[E]

    records = []
    for form in args.forms.split(","):
        for hd in args.hd.split(","):
            h, d = (int(x) for x in hd.split("x"))
            g = graph(args.edge_edges if form == "gatv2_edge" else args.edges)
            fns = _case(form, g, h, d, args.seed, dev)
            got = {n: fn() for n, fn in fns.items() if n != "forward"}
            torch.cuda.synchronize()
            diff = _rel(got["weights"], got["composed"])
            del got
            rec = {"form": form, "h": h, "d": d, "n_nodes": args.nodes, "n_edges": g.n_edges,
                   "chunk_size": args.chunk_size, "warmup": args.warmup, "iters": args.iters,
                   "times": _summary(_timed(fns, args.warmup, args.iters)),
                   "peak_added_bytes": _peaks(fns), "max_rel_diff_weights_vs_composed": diff,
                   "profile": {n: _profile(fn, 3) for n, fn in fns.items() if n != "composed"}}
            t = rec["times"]
            rec["weights_over_forward"] = round(t["weights"]["median_ms"] / t["forward"]["median_ms"], 3)
            rec["weights_over_composed"] = round(t["weights"]["median_ms"] / t["composed"]["median_ms"], 3)
            print(json.dumps(rec), flush=True)
            records.append(rec)
            del fns
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
