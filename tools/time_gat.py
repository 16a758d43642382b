#!/usr/bin/env python3
"""Time the GAT additive attention scores (graphop.gat_scores_forward / _backward) on the Reddit shape against the
workaround the library offered before them: maskedmm_csr at d = 2 on A = [el, 1], B = [1, er], torch's leaky_relu
forward and backward over the E x h scores, the gradients sliced out of dA / dB.

Both forms are first checked at full size: y against each other, del / der against a float64 sum (error per node
scaled by its sum of |g|).  Then, in one process and alternating, device events time: the new forward, the new
backward, the new forward + backward, and the workaround forward + backward (--warmup untimed rounds, median and min of --iters).  A separate profiled round reads
the library's per-launch times of the three kernels.  One JSON line per h; each names the algorithmic bytes of every
kernel with the convention of the headline metric (int64 ids at 8 B, values at 4 B, node tables once per pass):
E (16 + 4h) + 4h (n_src + n_dst) + 16 C, and the fraction of 8 TB/s they reach."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", default="reddit", choices=sorted(graphs.SHAPES))
    ap.add_argument("--heads", default="1,8")
    ap.add_argument("--slope", type=float, default=0.2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk-size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, E = graphs.SHAPES[args.shape]
    g = graphs.chung_lu_graph(N, E, alpha=0.5, seed=args.seed, chunk_size=args.chunk_size, device=dev)
    a8 = g.csr_args()
    s = args.slope
    n_src, n_dst = g.n_src, g.n_dst
    for h in (int(x) for x in args.heads.split(",")):
        gen = torch.Generator(device=dev).manual_seed(args.seed + h)
        shp = (lambda n: (n,) if h == 1 else (n, h))
        el = torch.randn(shp(g.n_src), generator=gen, device=dev)
        er = torch.randn(shp(g.n_dst), generator=gen, device=dev)
        dy = torch.randn(shp(g.n_edges), generator=gen, device=dev)
        # the workaround's operands: A = [el, 1], B = [1, er] as (n, 2) / (n, h, 2) rows of d = 2
        one_l, one_r = torch.ones_like(el), torch.ones_like(er)
        A = torch.stack([el, one_l], dim=-1).contiguous()
        B = torch.stack([one_r, er], dim=-1).contiguous()

        def new_fwd():
            return ops.gat_scores_forward(*a8[:4], el, er, s)

        def new_bwd():
            return ops.gat_scores_backward(*a8, el, er, dy, s)

        def new_both():
            new_fwd()
            return new_bwd()

        def workaround():
            z = ops.maskedmm_csr_forward(*a8[:4], A, B)
            y = F.leaky_relu(z, s)
            dz = torch.ops.aten.leaky_relu_backward(dy, z, s, False)
            dA, dB = ops.maskedmm_csr_backward(*a8, A, B, dz)
            return y, dA[..., 0], dB[..., 1]

        y0 = new_fwd()
        d_el, d_er = new_bwd()
        y1, w_el, w_er = workaround()
        torch.cuda.synchronize()
        y_equal = bool(torch.equal(y0, y1))
        torch.testing.assert_close(y0, y1, rtol=1e-6, atol=1e-6, msg=lambda m: "y: " + m)
        # del / der: both forms sum up to thousands of fp32 terms per node in different orders; each is held against a
        # float64 sum, its error scaled by the node's sum of |g| (the size of an fp32 accumulation error)
        z = el.double()[g.src] + er.double()[g.dst]
        gg = torch.where(z > 0, dy.double(), dy.double() * s)
        err = {}
        for name, idx, n, got in (("del", g.src, n_src, (d_el, w_el)), ("der", g.dst, n_dst, (d_er, w_er))):
            ref = torch.zeros((n,) + tuple(gg.shape[1:]), dtype=torch.float64, device=dev).index_add_(0, idx, gg)
            scale = torch.zeros_like(ref).index_add_(0, idx, gg.abs()) + 1e-30
            err[name] = [float(((x.double() - ref).abs() / scale).max()) for x in got]
            assert err[name][0] < 1e-5, (name, err[name])
            torch.testing.assert_close(got[0], got[1], rtol=1e-3, atol=1e-3, msg=lambda m: name + ": " + m)
        del y0, d_el, d_er, y1, w_el, w_er, z, gg

        t = _timed({"gat_fwd": new_fwd, "gat_bwd": new_bwd, "gat_fwd_bwd": new_both, "workaround_fwd_bwd": workaround},
                   args.warmup, args.iters)
        stats = {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)} for n, v in t.items()}

        # per-kernel times from the library's launch profile (events around each launch), in a round of their own
        _lib.profile_enable(True)
        try:
            _lib.profile_read()
            for _ in range(args.iters):
                new_fwd()
                new_bwd()
            prof = _lib.profile_read()
        finally:
            _lib.profile_enable(False)
        base = E * (16 + 4 * h) + 4 * h * (n_src + n_dst)
        kernels = {}
        for tag, chunks in (("gat_fwd", g.n_row_chunks), ("gat_bwd_row", g.n_row_chunks), ("gat_bwd_col", g.n_col_chunks)):
            p = prof[tag]
            nbytes = base + 16 * chunks
            kernels[tag] = {"kernel": p["kernel"], "calls": p["calls"], "mean_ms": round(p["mean_ms"], 4),
                            "min_ms": round(p["min_ms"], 4), "algorithmic_bytes": nbytes,
                            "fraction_of_8TBs": round(nbytes / (p["mean_ms"] * 1e-3) / PEAK, 3)}
        ours, theirs = stats["gat_fwd_bwd"]["median_ms"], stats["workaround_fwd_bwd"]["median_ms"]
        print(json.dumps({
            "tool": "tools/time_gat.py", "shape": args.shape, "n_src": n_src, "n_dst": n_dst, "n_edges": E,
            "row_chunks": g.n_row_chunks, "col_chunks": g.n_col_chunks, "chunk_size": args.chunk_size, "h": h,
            "negative_slope": s, "warmup": args.warmup, "iters": args.iters, "y_bitwise_equal_to_workaround": y_equal,
            "grad_error_vs_float64_new_and_workaround": err,
            "timings": stats, "speedup_fwd_bwd_vs_workaround": round(theirs / ours, 3), "kernels": kernels,
            "device": torch.cuda.get_device_name(dev)}), flush=True)
        del el, er, dy, A, B, one_l, one_r
        torch.cuda.empty_cache()
    _lib.check_errors()


if __name__ == "__main__":
    main()
