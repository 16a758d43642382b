#!/usr/bin/env python3
"""Time the fused attention step on bfloat16 tables (kernels_attn_bf16.h) against the fp32 step of the
same build, alternating in one process:

  * bf16: functions.fused_attention_step on bfloat16 leaves -- one call, the k_attn_bf16_* kernels;
  * fp32: the same step on the same values in float32 with the knob attn_heads = 1 -- the several-head kernels for
          8 x 32 and 4 x 64, the one-head fused passes for 1 x 64, and for 8 x 64, which has no fused fp32 form, head
          groups or (where groups would not save memory) the composed path; the record names which.

For every shape of --shapes and pair of --hd: --warmup untimed rounds, then the median, minimum and maximum of --iters
rounds by device events (the spread of the rounds is what a difference between the two has to exceed).  Before that the
bf16 step is checked against the fp32 one at full size (the largest error of a tensor over its largest value: the bf16
backward takes D = <dO, o> from the ROUNDED o, so a row of one edge, whose exact dQ is 0, gets a gradient of the size of
that rounding and no per-node scale applies; the tests compare against a reference given the same o) and the peak memory
each step adds to what is allocated before it is read from torch.cuda.max_memory_allocated.  A profiled round of its own
gives the library's per-launch times of the bf16 step.  One record per (shape, h, d), printed as a JSON line and
collected in --out (default profiles/fused_attention_bf16_bench.json)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from custom_op_benchmark_amd import _lib, functions, graphs, graphop as ops  # noqa: E402
from time_fused_attention_dropout import _profiled, _timed  # noqa: E402


def _tensor_err(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="reddit,products")
    ap.add_argument("--hd", default="8x32,4x64,1x64,8x64", help="comma-separated h x d pairs")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk-size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_attention_bf16_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    records = []
    for shape in args.shapes.split(","):
        N, E = graphs.SHAPES[shape]
        g = graphs.chung_lu_graph(N, E, alpha=0.5, seed=args.seed, chunk_size=args.chunk_size, device=dev)
        for hd in args.hd.split(","):
            h, d = (int(x) for x in hd.split("x"))
            gen = torch.Generator(device=dev).manual_seed(args.seed + h * 100 + d)
            # bf16 values, so that both steps compute on the same numbers
            vals = [(torch.randn((n, h, d), generator=gen, device=dev) / d ** 0.25).bfloat16()
                    for n in (g.n_src, g.n_dst, g.n_dst, g.n_src)]
            leaves = {torch.bfloat16: [x.clone().requires_grad_(True) for x in vals[:3]],
                      torch.float32: [x.float().requires_grad_(True) for x in vals[:3]]}
            dO = {torch.bfloat16: vals[3], torch.float32: vals[3].float()}
            del vals

            def step(dtype):
                def run():
                    for x in leaves[dtype]:
                        x.grad = None
                    _lib.tune("attn_heads", 1)
                    return functions.fused_attention_step(g, *leaves[dtype], dO[dtype])
                return run

            fns = {"bf16": step(torch.bfloat16), "fp32": step(torch.float32)}
            # full-size check (also builds and caches the plans both steps use)
            out = {}
            for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
                o = fns[name]().detach()
                out[name] = [o] + [x.grad.clone() for x in leaves[dtype]]
            torch.cuda.synchronize()
            err = {n: _tensor_err(x, y) for n, x, y in zip(("o", "dQ", "dK", "dV"), out["bf16"], out["fp32"])}
            assert all(v < 2e-2 for v in err.values()), err
            del out, o

            # what the fp32 step ran: one fused call, head groups (each through the one-head forms), or the composed path
            Qf, Kf = leaves[torch.float32][:2]
            hg = functions._heads_per_call(g.csr_args(), Qf, Kf, h)
            if ops.attention_backward_is_fused(*g.csr_args(), Qf, Kf):
                fp32_form = "several-head kernels" if h > 1 else "one-head fused passes"
            else:
                fp32_form = "head groups of %d" % hg if hg < h else "composed (unfused ops)"

            peak = {}
            for name, fn in fns.items():
                for x in leaves[torch.bfloat16] + leaves[torch.float32]:
                    x.grad = None
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                o = fn()
                torch.cuda.synchronize()
                peak[name] = torch.cuda.max_memory_allocated() - base
                del o

            t = _timed(fns, args.warmup, args.iters)
            timings = {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                           "max_ms": round(max(v), 4)} for n, v in t.items()}
            rec = {
                "tool": "tools/time_fused_attention_bf16.py", "shape": shape, "n_src": g.n_src, "n_dst": g.n_dst,
                "n_edges": E, "chunk_size": args.chunk_size, "h": h, "d": d, "warmup": args.warmup, "iters": args.iters,
                "fp32_form": fp32_form,
                "max_error_over_max_value_vs_fp32": err, "timings": timings,
                "bf16_over_fp32": round(timings["bf16"]["median_ms"] / timings["fp32"]["median_ms"], 3),
                "peak_added_bytes": peak, "peak_bf16_over_fp32": round(peak["bf16"] / peak["fp32"], 3),
                "kernels_bf16": _profiled(fns["bf16"], args.iters), "device": torch.cuda.get_device_name(dev)}
            print(json.dumps(rec), flush=True)
            records.append(rec)
            del leaves, dO, fns
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
