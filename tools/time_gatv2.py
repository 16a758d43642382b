#!/usr/bin/env python3
"""Time the GATv2 attention scores (graphop.gatv2_scores_forward / _backward) on the Reddit shape.

Yardsticks, timed in the same process and alternating with the op (device events; --warmup untimed rounds, median and
min of --iters):
  * the torch workaround the library offered before the op: (leaky_relu(xl[src] + xr[dst], s) * att).sum(-1) under
    autograd, on the same device.  It needs several (E, h, d) tensors (29 GB each at h d = 64 on the Reddit shape); where
    free memory is short it runs on a Chung-Lu graph of the same N with E cut until about six of them fit, the op is
    timed on that graph too, and the line records the size.  On that graph the two forms are also checked against each
    other.
  * k_gat_attn_bwd_row_f32 of the fused GAT layer at the same (h, d): the same driver with the same one-row-per-slot
    gather (launch profile of graphop.gat_attention_backward).
  * maskedmm_csr forward + backward at the same (h, d), for orientation: the same rows on the window / walk drivers.
A profiled round of its own reads the library's per-launch times of the three GATv2 kernels.  One JSON line per (h, d);
each kernel carries its gathered-row bytes (E h d 4 per pass) and its algorithmic bytes (DESIGN.md 4.6 convention: int64
ids at 8 B, values at 4 B, node tables once per pass) as fractions of 8 TB/s."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from custom_op_benchmark_amd import _lib, graphop as ops, graphs  # noqa: E402

PEAK = 8e12


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


def _stats(t):
    return {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)} for n, v in t.items()}


def _operands(g, h, d, seed, dev):
    gen = torch.Generator(device=dev).manual_seed(seed)
    node = (lambda n: (n, d) if h == 1 else (n, h, d))
    xl = torch.randn(node(g.n_src), generator=gen, device=dev)
    xr = torch.randn(node(g.n_dst), generator=gen, device=dev)
    att = torch.randn(node(1)[1:], generator=gen, device=dev) / d ** 0.5
    dy = torch.randn((g.n_edges,) if h == 1 else (g.n_edges, h), generator=gen, device=dev)
    return xl, xr, att, dy


def _op_fns(g, xl, xr, att, dy, s):
    a8 = g.csr_args()

    def fwd():
        return ops.gatv2_scores_forward(*a8[:4], xl, xr, att, s)

    def bwd():
        return ops.gatv2_scores_backward(*a8, xl, xr, att, dy, s)

    def both():
        fwd()
        return bwd()
    return fwd, bwd, both


def _workaround(g, xl, xr, att, dy, s):
    """the torch route under autograd: -> (y, dxl, dxr, datt)"""
    l, r, a = (t.detach().requires_grad_(True) for t in (xl, xr, att))
    y = (F.leaky_relu(l[g.src] + r[g.dst], s) * a).sum(-1)
    y.backward(dy)
    return y.detach(), l.grad, r.grad, a.grad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", default="reddit", choices=sorted(graphs.SHAPES))
    ap.add_argument("--pairs", default="1x64,8x8,8x32", help="(h, d) pairs as HxD, comma separated")
    ap.add_argument("--slope", type=float, default=0.2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk-size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--workaround-tensors", type=float, default=6.0,
                    help="(E, h, d) tensors the torch workaround is given room for, out of 80 %% of the free memory")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_gatv2.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    N, E = graphs.SHAPES[args.shape]
    s = args.slope
    g = graphs.chung_lu_graph(N, E, alpha=0.5, seed=args.seed, chunk_size=args.chunk_size, device=dev)
    n_src, n_dst = g.n_src, g.n_dst
    small = {}          # cut graphs for the workaround, by edge count
    for h, d in (tuple(int(x) for x in p.split("x")) for p in args.pairs.split(",")):
        xl, xr, att, dy = _operands(g, h, d, args.seed + 100 * h + d, dev)
        fwd, bwd, both = _op_fns(g, xl, xr, att, dy, s)
        both()
        torch.cuda.synchronize()

        # the other two yardsticks' operands: the fused GAT layer's (el, er, V, dO) and maskedmm's dy
        gen = torch.Generator(device=dev).manual_seed(args.seed + 7)
        el = torch.randn((n_src,) if h == 1 else (n_src, h), generator=gen, device=dev)
        er = torch.randn((n_dst,) if h == 1 else (n_dst, h), generator=gen, device=dev)
        a8 = g.csr_args()

        def mm_both():
            ops.maskedmm_csr_forward(*a8[:4], xl, xr)
            return ops.maskedmm_csr_backward(*a8, xl, xr, dy)

        t = _stats(_timed({"gatv2_fwd": fwd, "gatv2_bwd": bwd, "gatv2_fwd_bwd": both, "maskedmm_fwd_bwd": mm_both},
                          args.warmup, args.iters))

        # per-kernel times from the library's launch profile (events around each launch), in a round of their own;
        # the fused GAT layer's backward at the same (h, d) runs in the same round
        o, stats = ops.gat_attention_forward(*a8[:4], el, er, xr, s)
        dO = xl if n_src == n_dst else torch.randn_like(o)
        _lib.profile_enable(True)
        try:
            _lib.profile_read()
            for _ in range(args.iters):
                fwd()
                bwd()
                ops.gat_attention_backward(*a8, el, er, xr, o, stats, dO, s)
            prof = _lib.profile_read()
        finally:
            _lib.profile_enable(False)
        del o, stats, el, er
        gathered = E * h * d * 4
        ids = 16 * E
        tables = 4 * h * d * (n_src + n_dst)
        alg = {"gatv2_fwd": ids + 4 * h * E + tables + 16 * g.n_row_chunks,
               "gatv2_bwd_row": ids + 4 * h * E + tables + 4 * h * d * n_src + 16 * g.n_row_chunks,
               "gatv2_bwd_col": ids + 4 * h * E + tables + 4 * h * d * n_dst + 16 * g.n_col_chunks}
        kernels = {}
        for tag, nbytes in alg.items():
            p = prof[tag]
            sec = p["mean_ms"] * 1e-3
            kernels[tag] = {"kernel": p["kernel"], "calls": p["calls"], "mean_ms": round(p["mean_ms"], 4),
                            "min_ms": round(p["min_ms"], 4), "gathered_row_bytes": gathered,
                            "gathered_fraction_of_8TBs": round(gathered / sec / PEAK, 3), "algorithmic_bytes": nbytes,
                            "algorithmic_fraction_of_8TBs": round(nbytes / sec / PEAK, 3)}
        p = prof["gat_attn_bwd_row"]
        yard = {"kernel": p["kernel"], "mean_ms": round(p["mean_ms"], 4), "min_ms": round(p["min_ms"], 4)}
        ratio = {tag: round(kernels[tag]["mean_ms"] / p["mean_ms"], 3) for tag in kernels}

        # the torch workaround, on a graph it fits (halved again if the allocator still runs out)
        free = torch.cuda.mem_get_info(dev)[0]
        e_w = min(E, int(0.8 * free / (args.workaround_tensors * h * d * 4)))
        while True:
            if e_w >= E:
                gw, e_w = g, E
                wl, wr, wa, wdy = xl, xr, att, dy
            else:
                e_w = max(1 << 20, (e_w >> 20) << 20)
                if e_w not in small:
                    small[e_w] = graphs.chung_lu_graph(N, e_w, alpha=0.5, seed=args.seed, chunk_size=args.chunk_size,
                                                       device=dev)
                gw = small[e_w]
                wl, wr, wa, wdy = _operands(gw, h, d, args.seed + 100 * h + d, dev)
            wfwd, wbwd, wboth = _op_fns(gw, wl, wr, wa, wdy, s)

            def torch_both():
                return _workaround(gw, wl, wr, wa, wdy, s)

            # the two forms against each other (fp32 both: twice the project's band; datt relative to its largest entry)
            y0 = wfwd()
            g0 = wbwd()
            try:
                y1, *g1 = torch_both()
            except torch.cuda.OutOfMemoryError:
                del y0, g0
                torch.cuda.empty_cache()
                assert e_w > (1 << 20), "the torch workaround does not fit at any size"
                e_w //= 2
                continue
            break
        torch.testing.assert_close(y0, y1, rtol=2e-4, atol=2e-5, msg=lambda m: "y: " + m)
        for name, u, v in zip(("dxl", "dxr"), g0, g1):
            torch.testing.assert_close(u, v, rtol=2e-4, atol=1e-3, msg=lambda m: name + ": " + m)
        datt_rel = float(((g0[2] - g1[2]).abs() / g1[2].abs().max()).max())
        assert datt_rel < 1e-3, datt_rel
        del y0, g0, y1, g1
        torch.cuda.empty_cache()
        tw = _stats(_timed({"gatv2_fwd_bwd": wboth, "torch_fwd_bwd": torch_both}, args.warmup, args.iters))
        line = {
            "tool": "tools/time_gatv2.py", "shape": args.shape, "n_src": n_src, "n_dst": n_dst, "n_edges": E,
            "row_chunks": g.n_row_chunks, "col_chunks": g.n_col_chunks, "chunk_size": args.chunk_size, "h": h, "d": d,
            "negative_slope": s, "warmup": args.warmup, "iters": args.iters, "timings": t, "kernels": kernels,
            "gat_attn_bwd_row_same_shape": yard, "kernel_time_over_gat_attn_bwd_row": ratio,
            "maskedmm_fwd_bwd_over_gatv2_fwd_bwd": round(t["maskedmm_fwd_bwd"]["median_ms"] / t["gatv2_fwd_bwd"]["median_ms"], 3),
            "workaround": {"n_edges": e_w, "full_size": e_w == E, "free_bytes_before": free, "timings": tw,
                           "datt_max_diff_over_max": datt_rel,
                           "speedup_fwd_bwd_vs_torch": round(tw["torch_fwd_bwd"]["median_ms"] / tw["gatv2_fwd_bwd"]["median_ms"], 3)},
            "device": torch.cuda.get_device_name(dev)}
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
        assert tw["gatv2_fwd_bwd"]["median_ms"] < tw["torch_fwd_bwd"]["median_ms"], "the bar: faster than the torch workaround"
        del xl, xr, att, dy, wl, wr, wa, wdy
        torch.cuda.empty_cache()
    _lib.check_errors()


if __name__ == "__main__":
    main()
