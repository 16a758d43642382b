#!/usr/bin/env python3
"""Time the fused dot-product attention step with attention dropout (functions.fused_attention_dropout_step:
FusedAttentionDropout) on the Reddit shape against its two yardsticks:

  * the fused step WITHOUT dropout (functions.fused_attention_step), whose kernels are the undropped instantiations --
    the ratio says what recomputing the Philox decision per slot costs next to the dot products;
  * the composed dropout step (functions.attention_dropout_step: MaskedMMCSR -> SparseSoftmax -> * edge_dropout_mask ->
    VectorSPMM), which keeps a, the mask and their product as (E, h) tensors.

All three alternate in one process: --warmup untimed rounds, then the median and minimum of --iters rounds by device
events.  Before that the fused dropout step is checked against the composed one at full size (o, dQ, dK, dV, the error of
every node scaled by the node's largest value in the composed result), and the peak memory each step adds to what is
allocated before it is read from torch.cuda.max_memory_allocated.  A profiled round of their own gives the library's
per-launch times of the fused step with and without dropout, pass by pass.  One record per (h, d), printed as a JSON
line and collected in --out (default profiles/fused_attention_dropout_bench.json)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from custom_op_benchmark_amd import _lib, functions, graphs  # noqa: E402


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


def _profiled(fn, iters):
    _lib.profile_enable(True)
    try:
        _lib.profile_read()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        prof = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    return {t: {"kernel": r["kernel"], "calls": r["calls"], "mean_ms": round(r["mean_ms"], 4), "min_ms": round(r["min_ms"], 4)}
            for t, r in prof.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", default="reddit", choices=sorted(graphs.SHAPES))
    ap.add_argument("--hd", default="1x64,8x32", help="comma-separated h x d pairs")
    ap.add_argument("--p", type=float, default=0.5)
    ap.add_argument("--dropout-seed", type=int, default=1234567890123)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk-size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_attention_dropout_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, E = graphs.SHAPES[args.shape]
    g = graphs.chung_lu_graph(N, E, alpha=0.5, seed=args.seed, chunk_size=args.chunk_size, device=dev)
    drop = (args.p, args.dropout_seed, 7)
    records = []
    for hd in args.hd.split(","):
        h, d = (int(x) for x in hd.split("x"))
        gen = torch.Generator(device=dev).manual_seed(args.seed + h * 100 + d)
        vs = (lambda n: (n, d) if h == 1 else (n, h, d))
        Q, K, V = (((torch.randn(vs(n), generator=gen, device=dev)) / d ** 0.25).requires_grad_(True)
                   for n in (g.n_src, g.n_dst, g.n_dst))
        dO = torch.randn(vs(g.n_src), generator=gen, device=dev)
        leaves = (Q, K, V)

        def step(fn, *extra):
            def run():
                for x in leaves:
                    x.grad = None
                return fn(g, Q, K, V, dO, *extra)
            return run

        fused = step(functions.fused_attention_dropout_step, *drop)
        nodrop = step(functions.fused_attention_step)
        composed = step(functions.attention_dropout_step, *drop)

        # full-size check (also builds and caches the plans all steps use)
        o_c = composed()[2].detach()
        want = [o_c] + [x.grad.clone() for x in leaves]
        o_f = fused().detach()
        got = [o_f] + [x.grad.clone() for x in leaves]
        torch.cuda.synchronize()
        err = {n: _node_err(x, y) for n, x, y in zip(("o", "dQ", "dK", "dV"), got, want)}
        assert all(v < 1e-3 for v in err.values()), err
        del o_c, o_f, want, got
        nodrop()

        peak = {}
        for name, fn in (("fused_dropout", fused), ("fused_no_dropout", nodrop), ("composed_dropout", composed)):
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

        t = _timed({"fused_dropout": fused, "fused_no_dropout": nodrop, "composed_dropout": composed}, args.warmup,
                   args.iters)
        timings = {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)} for n, v in t.items()}
        f, n0, c = (timings[k]["median_ms"] for k in ("fused_dropout", "fused_no_dropout", "composed_dropout"))
        rec = {
            "tool": "tools/time_fused_attention_dropout.py", "shape": args.shape, "n_src": g.n_src, "n_dst": g.n_dst,
            "n_edges": E, "chunk_size": args.chunk_size, "h": h, "d": d,
            "dropout": {"p": drop[0], "seed": drop[1], "offset": drop[2]}, "warmup": args.warmup, "iters": args.iters,
            "node_scaled_error_vs_composed": err, "timings": timings,
            "fused_dropout_over_fused_no_dropout": round(f / n0, 3), "fused_dropout_over_composed_dropout": round(f / c, 3),
            "peak_added_bytes": peak, "one_edge_tensor_bytes": E * h * 4,
            "kernels_fused_dropout": _profiled(fused, args.iters), "kernels_fused_no_dropout": _profiled(nodrop, args.iters),
            "device": torch.cuda.get_device_name(dev)}
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del Q, K, V, dO, leaves
        torch.cuda.empty_cache()
    _lib.check_errors()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(records, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
