#!/usr/bin/env python3
"""Time the fused GATv2 attention step on bfloat16 tables against the fp32 fused step of the same build,
alternating in one process: device events around each fwd+bwd, --warmup untimed rounds, median and range of --iters.
--dropout P times the attention-dropout forms of both.  The bf16 step is first checked against the fp32 fused step on
the widened inputs (node-scaled, one bf16 rounding).  A separate profiled round reads the library's per-launch times of
the gather passes of both steps and puts the byte model of 4.5u beside them: per slot the gathered rows (2 or 4 bytes an
element; two rows in bwd_col), the 8-byte id, and in bwd_col the 16 h-byte P item.  One JSON line per (h, d)."""
import argparse
import json
import os
import statistics
import sys

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from custom_op_benchmark_amd import _lib, functions, graphs  # noqa: E402
from time_fused_gat import _node_err, _timed  # noqa: E402

PASSES = ("fwd", "bwd_row", "bwd_col")


def _slot_bytes(h, d, es):
    """bytes per slot of the three gather passes at element size es"""
    row, ident = h * d * es, 8
    return {"fwd": row + ident, "bwd_row": row + ident, "bwd_col": 2 * row + 16 * h + ident}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", default="reddit", choices=sorted(graphs.SHAPES))
    ap.add_argument("--hd", default="1x64,8x8,8x32", help="comma-separated h x d pairs")
    ap.add_argument("--slope", type=float, default=0.2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk-size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dropout", type=float, default=0.0, metavar="P")
    ap.add_argument("--dropout-seed", type=int, default=1234567890123)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, E = graphs.SHAPES[args.shape]
    g = graphs.chung_lu_graph(N, E, alpha=0.5, seed=args.seed, chunk_size=args.chunk_size, device=dev)
    s, p = args.slope, args.dropout
    drop = (p, args.dropout_seed, 7)
    for hd in args.hd.split(","):
        h, d = (int(x) for x in hd.split("x"))
        gen = torch.Generator(device=dev).manual_seed(args.seed + h * 100 + d)
        vs = (lambda n: (n, d) if h == 1 else (n, h, d))
        xl, xr, dO = (torch.randn(vs(n), generator=gen, device=dev) for n in (g.n_src, g.n_dst, g.n_src))
        att = torch.randn(vs(1)[1:], generator=gen, device=dev) / d ** 0.5
        bf = [x.bfloat16() for x in (xl, xr, att, dO)]
        leaves16 = [x.clone().requires_grad_(True) for x in bf[:3]]
        leaves32 = [x.float().requires_grad_(True) for x in bf[:3]]          # the widened inputs
        dO16, dO32 = bf[3], bf[3].float()
        del xl, xr, dO

        def step(leaves, dO_):
            for x in leaves:
                x.grad = None
            return functions.fused_gatv2_attention_dropout_step(g, *leaves, dO_, *drop, s) if p else \
                functions.fused_gatv2_attention_step(g, *leaves, dO_, s)

        o32 = step(leaves32, dO32).detach()
        o16 = step(leaves16, dO16).detach()
        torch.cuda.synchronize()
        err = {"o": _node_err(o16, o32)}
        for name, x, y in zip(("dxl", "dxr", "datt"), leaves16, leaves32):
            err[name] = float((x.grad.double() - y.grad.double()).abs().max() / (y.grad.double().abs().max() + 1e-30))
        assert err["o"] < 2 ** -7, err          # (the gradients: reported; D_i comes from the rounded o)
        del o32, o16

        fns = {"bf16_fused": lambda: step(leaves16, dO16), "fp32_fused": lambda: step(leaves32, dO32)}
        t = _timed(fns, args.warmup, args.iters)
        timings = {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
                   for n, v in t.items()}

        kernels = {}
        for name in fns:
            _lib.profile_enable(True)
            try:
                _lib.profile_read()
                for _ in range(args.iters):
                    fns[name]()
                torch.cuda.synchronize()
                prof = _lib.profile_read()
            finally:
                _lib.profile_enable(False)
            kernels[name] = {tag: {"kernel": r["kernel"], "calls": r["calls"], "mean_ms": round(r["mean_ms"], 4),
                                   "min_ms": round(r["min_ms"], 4)}
                             for tag, r in sorted(prof.items()) if "gv2attn" in tag or "gatv2_attn_bf16" in tag}
        b16, b32 = _slot_bytes(h, d, 2), _slot_bytes(h, d, 4)
        passes = {}
        for ps in PASSES:
            k32 = kernels["fp32_fused"][("gv2attn_drop_" if p else "gv2attn_") + ps]
            k16 = kernels["bf16_fused"]["gatv2_attn_bf16_" + ps]
            passes[ps] = {"bf16_ms": k16["mean_ms"], "fp32_ms": k32["mean_ms"],
                          "measured_ratio": round(k16["mean_ms"] / k32["mean_ms"], 3),
                          "byte_model_ratio": round(b16[ps] / b32[ps], 3),
                          "bf16_slot_bytes_fraction_of_8TBs": round(E * b16[ps] / (k16["mean_ms"] * 1e-3) / 8e12, 3)}
        med = {n: v["median_ms"] for n, v in timings.items()}
        print(json.dumps({
            "tool": "tools/time_fused_gatv2_bf16.py", "shape": args.shape, "n_src": g.n_src, "n_dst": g.n_dst, "n_edges": E,
            "chunk_size": args.chunk_size, "h": h, "d": d, "negative_slope": s, "dropout_p": p, "warmup": args.warmup,
            "iters": args.iters, "node_scaled_error_vs_fp32_fused": err, "timings": timings,
            "bf16_fused_over_fp32_fused": round(med["bf16_fused"] / med["fp32_fused"], 3),
            "gather_passes": passes, "kernels": kernels, "device": torch.cuda.get_device_name(dev)}), flush=True)
        del bf, leaves16, leaves32, dO16, dO32
        torch.cuda.empty_cache()
    _lib.check_errors()


if __name__ == "__main__":
    main()
