#!/usr/bin/env python3
"""Time the several-head form of the fused dot-product attention step (kernels_attn_heads.h) on the
Reddit shape against the two forms it replaces, alternating in one process:

  * heads   : the fused step with the knob attn_heads = 1 -- one call for all heads, the several-head kernels;
  * groups  : the same step with attn_heads = 0 -- head groups (functions._head_group), each group through the composed
              path or the one-head kernels: what the step was before the several-head kernels existed;
  * composed: the 8-function step that keeps its (E, h) tensors (functions.attention_bias_step / attention_dropout_step /
              attention_step).

For every (h, d) the step with a bias runs at every p of --p, and once without a bias (p = 0).  --warmup untimed rounds,
then the median, minimum and maximum of --iters rounds by device events (the spread of the rounds is what a difference
between two forms has to exceed).  Before that the heads step is checked against the composed one at full size (the
error of every node scaled by the node's largest value in the composed result, db as one row) and the peak memory each
step adds to what is allocated before it is read from torch.cuda.max_memory_allocated.  A profiled round of its own
gives the library's per-launch times of the heads step.  One record per (h, d, bias, p), printed as a JSON line and
collected in --out (default profiles/fused_attention_heads_bench.json)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from custom_op_benchmark_amd import _lib, functions, graphs  # noqa: E402
from time_fused_attention_dropout import _node_err, _profiled, _timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", default="reddit", choices=sorted(graphs.SHAPES))
    ap.add_argument("--hd", default="8x32,4x64", help="comma-separated h x d pairs")
    ap.add_argument("--p", default="0,0.5", help="comma-separated dropout probabilities of the step with a bias")
    ap.add_argument("--dropout-seed", type=int, default=1234567890123)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk-size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_attention_heads_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, E = graphs.SHAPES[args.shape]
    g = graphs.chung_lu_graph(N, E, alpha=0.5, seed=args.seed, chunk_size=args.chunk_size, device=dev)
    records = []
    for hd in args.hd.split(","):
        h, d = (int(x) for x in hd.split("x"))
        gen = torch.Generator(device=dev).manual_seed(args.seed + h * 100 + d)
        Q, K, V = ((torch.randn((n, h, d), generator=gen, device=dev) / d ** 0.25).requires_grad_(True)
                   for n in (g.n_src, g.n_dst, g.n_dst))
        b = torch.randn((g.n_edges, h), generator=gen, device=dev).requires_grad_(True)
        dO = torch.randn((g.n_src, h, d), generator=gen, device=dev)
        leaves = (Q, K, V, b)

        def step(knob, fn, *extra):
            def run():
                for x in leaves:
                    x.grad = None
                _lib.tune("attn_heads", knob)
                return fn(g, Q, K, V, *extra)
            return run

        cases = [(True, float(x)) for x in args.p.split(",")] + [(False, 0.0)]
        for bias, p in cases:
            drop = (p, args.dropout_seed, 7)
            if bias:
                fused_fn, fused_args = functions.fused_attention_bias_step, (b, dO) + drop
                comp_fn, comp_args = functions.attention_bias_step, (b, dO) + drop
            else:
                fused_fn, fused_args = functions.fused_attention_step, (dO,)
                comp_fn, comp_args = functions.attention_step, (dO,)
            heads, groups = step(1, fused_fn, *fused_args), step(0, fused_fn, *fused_args)
            composed = step(0, comp_fn, *comp_args)
            used = leaves if bias else leaves[:3]

            # full-size check (also builds and caches the plans all steps use)
            o_c = composed()[2].detach()
            want = [o_c] + [x.grad.clone() for x in used]
            o_h = heads().detach()
            got = [o_h] + [x.grad.clone() for x in used]
            torch.cuda.synchronize()
            err = {n: _node_err(x, y) for n, x, y in zip(("o", "dQ", "dK", "dV"), got, want)}
            if bias:
                err["db"] = _node_err(got[4].reshape(1, -1), want[4].reshape(1, -1))
            assert all(v < 1e-3 for v in err.values()), err
            del o_c, o_h, want, got
            groups()
            _lib.tune("attn_heads", -1)          # what the default rule chooses for this call
            auto = functions._heads_per_call(g.csr_args(), Q, K, h)

            fns = {"heads": heads, "groups": groups, "composed": composed}
            peak = {}
            for name, fn in fns.items():
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

            t = _timed(fns, args.warmup, args.iters)
            timings = {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                           "max_ms": round(max(v), 4)} for n, v in t.items()}
            hm, gm, cm = (timings[k]["median_ms"] for k in ("heads", "groups", "composed"))
            rec = {
                "tool": "tools/time_fused_attention_heads.py", "shape": args.shape, "n_src": g.n_src, "n_dst": g.n_dst,
                "n_edges": E, "chunk_size": args.chunk_size, "h": h, "d": d, "bias": bias,
                "dropout": {"p": drop[0], "seed": drop[1], "offset": drop[2]}, "warmup": args.warmup, "iters": args.iters,
                "node_scaled_error_vs_composed": err, "timings": timings,
                "heads_over_groups": round(hm / gm, 3), "heads_over_composed": round(hm / cm, 3),
                "auto_takes_the_heads_form": auto == h,
                "peak_added_bytes": peak, "peak_heads_over_groups": round(peak["heads"] / peak["groups"], 3),
                "one_edge_tensor_bytes": E * h * 4,
                "kernels_heads": _profiled(heads, args.iters), "device": torch.cuda.get_device_name(dev)}
            print(json.dumps(rec), flush=True)
            records.append(rec)
        del Q, K, V, b, dO, leaves
        torch.cuda.empty_cache()
    _lib.tune_reset()
    _lib.check_errors()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(records, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
