#!/usr/bin/env python3
"""Time the bfloat16 fused attention step with attention dropout, a per-edge score bias, or both (kernels_attn_bf16_opts.h,
DESIGN.md 4.5w) against the fp32 step of the same build with the same options and against the plain bf16 step, the three
alternating in one process:

  * bf16:  FusedAttentionDropout / FusedAttentionBias on bfloat16 leaves -- one call, the k_attnopt_bf16_* kernels;
  * fp32:  the same class on the same values in float32 with the knob attn_heads = 1 (the several-head kernels for
           8 x 32 and 4 x 64, the one-head fused passes for 1 x 64);
  * plain: functions.fused_attention_step on the bfloat16 leaves, no option.

For every shape of --shapes, pair of --hd and mode: --warmup untimed rounds, then the median, minimum and maximum of
--iters rounds by device events.  Before that the bf16 step is checked against the fp32 one at full size (the largest
error of a tensor over its largest value, as tools/time_fused_attention_bf16.py).  b.grad is wanted in both.  One
record per (shape, h, d, mode), printed as a JSON line and collected in --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from custom_op_benchmark_amd import _lib, functions, graphs  # noqa: E402
from time_fused_attention_bf16 import _tensor_err  # noqa: E402
from time_fused_attention_dropout import _profiled, _timed  # noqa: E402

MODES = {"dropout": (0.5, False), "bias": (0.0, True), "both": (0.5, True)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="reddit,products")
    ap.add_argument("--hd", default="8x32,4x64,1x64", help="comma-separated h x d pairs")
    ap.add_argument("--modes", default="dropout,bias,both")
    ap.add_argument("--dropout-seed", type=int, default=1234567890123)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk-size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_attention_bf16_opts_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    BF, F32 = torch.bfloat16, torch.float32
    records = []
    for shape in args.shapes.split(","):
        N, E = graphs.SHAPES[shape]
        g = graphs.chung_lu_graph(N, E, alpha=0.5, seed=args.seed, chunk_size=args.chunk_size, device=dev)
        for hd in args.hd.split(","):
            h, d = (int(x) for x in hd.split("x"))
            gen = torch.Generator(device=dev).manual_seed(args.seed + h * 100 + d)
            # bf16 values, so that both dtypes compute on the same numbers
            vals = [(torch.randn((n, h, d), generator=gen, device=dev) / d ** 0.25).bfloat16()
                    for n in (g.n_src, g.n_dst, g.n_dst, g.n_src)]
            vals.append(torch.randn((g.n_edges, h), generator=gen, device=dev).bfloat16())
            leaves = {BF: [x.clone().requires_grad_(True) for x in vals[:3] + vals[4:]],
                      F32: [x.float().requires_grad_(True) for x in vals[:3] + vals[4:]]}
            dO = {BF: vals[3], F32: vals[3].float()}
            del vals
            for mode in args.modes.split(","):
                p, biased = MODES[mode]

                def step(dtype, plain=False):
                    q, k, v, b = leaves[dtype]

                    def run():
                        for x in leaves[dtype]:
                            x.grad = None
                        _lib.tune("attn_heads", 1)
                        if plain:
                            return functions.fused_attention_step(g, q, k, v, dO[dtype])
                        if biased:
                            return functions.fused_attention_bias_step(g, q, k, v, b, dO[dtype], p, args.dropout_seed)
                        return functions.fused_attention_dropout_step(g, q, k, v, dO[dtype], p, args.dropout_seed)
                    return run

                fns = {"bf16": step(BF), "fp32": step(F32), "plain": step(BF, plain=True)}
                out = {}
                for name, dtype in (("fp32", F32), ("bf16", BF)):          # full-size check (also caches the plans)
                    o = fns[name]().detach()
                    out[name] = [o] + [x.grad.clone() for x in leaves[dtype][:4 if biased else 3]]
                torch.cuda.synchronize()
                err = {n: _tensor_err(x, y) for n, x, y in zip(("o", "dQ", "dK", "dV", "db"), out["bf16"], out["fp32"])}
                assert all(v < 2e-2 for v in err.values()), err
                del out, o
                t = _timed(fns, args.warmup, args.iters)
                timings = {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                               "max_ms": round(max(v), 4)} for n, v in t.items()}
                med = {n: timings[n]["median_ms"] for n in timings}
                rec = {"tool": "tools/time_fused_attention_bf16_opts.py", "shape": shape, "n_src": g.n_src, "n_dst": g.n_dst,
                       "n_edges": E, "chunk_size": args.chunk_size, "h": h, "d": d, "mode": mode, "p": p,
                       "warmup": args.warmup, "iters": args.iters, "max_error_over_max_value_vs_fp32": err,
                       "timings": timings, "bf16_over_fp32": round(med["bf16"] / med["fp32"], 3),
                       "bf16_over_plain_bf16": round(med["bf16"] / med["plain"], 3),
                       "kernels_bf16": _profiled(fns["bf16"], args.iters), "device": torch.cuda.get_device_name(dev)}
                print(json.dumps(rec), flush=True)
                records.append(rec)
                del fns
            del leaves, dO
            torch.cuda.empty_cache()
        del g
        _lib.clear_plan_cache()
        torch.cuda.empty_cache()
    _lib.tune_reset()
    _lib.check_errors()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(records, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
