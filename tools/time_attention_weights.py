#!/usr/bin/env python3
"""Time graphop.attention_weights (the weights of the fused dot-product attention ops from their row statistics,
DESIGN.md 4.5n) against the routes a user had before it.

Per (h, d), candidates alternate in one process, --warmup untimed rounds and then --iters rounds timed by device events:
  plain / bias   weights   attention_weights(Q, K, stats[, b]): the library's SDDMM + one (E, h) stream pass
                 composed  sparse_softmax_forward(maskedmm_csr_forward(Q, K) [+ b]): a second softmax (that route's code
                           is unchanged by the op)
  edge           weights   attention_weights(Q, K, stats, xe=xe): k_attn_weights_xe_f32, one gathered row per slot
                 forward   attention_edge_forward at the same shape, whose pass attn_edge_fwd_rows shares the driver and
                           gathers two rows per slot (its kernel time is read from the launch profile)
                 torch     (--torch-edges N > 0) on a graph cut to N edges, where the (E, h, d) temporaries of
                           softmax((Q[row] * (K[col] + xe)).sum(-1)) fit, next to `weights` on that graph
stats always come from the matching fused forward.  Reported: medians (min..max), the peak memory each candidate adds to
what is allocated before it, the per-kernel times of the library's launch profile (rounds of their own) next to the bytes
of the model of 4.5n -- norm pass: 4 h E read (+ 4 h E of b), 4 h E written, 8 E of eid unless identity, 16 C; xe pass:
4 E h d gathered, 4 E h d streamed, 4 h E written, 8 E + (8 E unless identity) + 16 C of ids -- and the largest relative
difference between the candidates' weights.  Nothing is asserted on a time.
Graph: chung_lu_graph(N of --shape, --edges or the shape's E, alpha=0.5, seed=--seed).  One JSON record per case, printed
and collected in --out (default profiles/attention_weights_bench.json; --append keeps the records already there)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from custom_op_benchmark_amd import _lib, graphs, graphop as ops  # noqa: E402

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


def _operands(g, h, d, seed, dev):
    gen = torch.Generator(device=dev).manual_seed(seed + h * 100 + d)
    ns = (lambda n: (n, d) if h == 1 else (n, h, d))
    Q = torch.randn(ns(g.n_src), generator=gen, device=dev) / d ** 0.5
    K, V = (torch.randn(ns(g.n_dst), generator=gen, device=dev) for _ in range(2))
    xe = torch.randn(ns(g.n_edges), generator=gen, device=dev)
    b = torch.randn((g.n_edges,) if h == 1 else (g.n_edges, h), generator=gen, device=dev)
    return Q, K, V, xe, b


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", default="reddit", choices=sorted(graphs.SHAPES))
    ap.add_argument("--edges", type=int, default=None, metavar="N", help="N edges instead of the shape's")
    ap.add_argument("--hd", default="1x64,8x8,8x32", help="comma-separated h x d pairs")
    ap.add_argument("--modes", default="plain,bias,edge")
    ap.add_argument("--torch-edges", type=int, default=2_000_000, metavar="N",
                    help="edges of the cut graph the torch route of the edge mode runs on (0: leave it out)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk-size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--append", action="store_true", help="keep the records --out already holds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_weights_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, E = graphs.SHAPES[args.shape]
    if args.edges:
        E = args.edges
    g = graphs.chung_lu_graph(N, E, alpha=0.5, seed=args.seed, chunk_size=args.chunk_size, device=dev)
    small = graphs.chung_lu_graph(N, args.torch_edges, alpha=0.5, seed=args.seed, chunk_size=args.chunk_size, device=dev) \
        if args.torch_edges else None
    a4 = g.csr_args()[:4]
    E, C = g.n_edges, g.n_row_chunks
    identity = bool(_lib.get_plan(*a4, g.n_dst).info.eid_identity)
    records = []
    if args.append and os.path.exists(args.out):
        with open(args.out) as fh:
            records = json.load(fh)

    def emit(rec):
        rec.update(tool="tools/time_attention_weights.py", shape=args.shape, warmup=args.warmup, iters=args.iters,
                   chunk_size=args.chunk_size, device=torch.cuda.get_device_name(dev))
        print(json.dumps(rec), flush=True)
        records.append(rec)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:      # rewritten after every case: a run that is cut short keeps what it has
            json.dump(records, fh, indent=1)
            fh.write("\n")

    for hd in args.hd.split(","):
        h, d = (int(x) for x in hd.split("x"))
        Q, K, V, xe, b = _operands(g, h, d, args.seed, dev)
        ids = 16 * C + (0 if identity else 8 * E)
        for mode in args.modes.split(","):
            head = {"graph": "chung_lu_graph(%d, %d, alpha=0.5, seed=%d)" % (N, E, args.seed), "n_q": g.n_src,
                    "n_k": g.n_dst, "n_edges": E, "row_chunks": C, "h": h, "d": d, "mode": mode, "eid_identity": identity}
            if mode == "edge":
                stats = ops.attention_edge_forward(*a4, Q, K, V, xe)[1]
                fns = {"weights": lambda: ops.attention_weights(*a4, Q, K, stats, None, xe),
                       "forward": lambda: ops.attention_edge_forward(*a4, Q, K, V, xe)}
                model = {"attn_weights_xe": 8 * E * h * d + 4 * E * h + 8 * E + ids}
                diff = None
            else:
                bb = b if mode == "bias" else None
                stats = (ops.attention_bias_forward(*a4, Q, K, V, bb) if bb is not None
                         else ops.attention_dropout_forward(*a4, Q, K, V))[1]

                def composed():
                    s = ops.maskedmm_csr_forward(*a4, Q, K)
                    if bb is not None:
                        s += bb
                    return ops.sparse_softmax_forward(*a4[:3], s)

                fns = {"weights": lambda: ops.attention_weights(*a4, Q, K, stats, bb), "composed": composed}
                model = {"attn_weights_norm": (3 if bb is not None else 2) * 4 * E * h + ids}
                diff = _rel(fns["weights"](), composed())
            peak = _peaks(fns)
            timings = _summary(_timed(fns, args.warmup, args.iters))
            kernels = {n: _profile(fn, args.iters) for n, fn in fns.items()}
            for tag, nbytes in model.items():
                q = kernels["weights"].get(tag)
                if q:
                    q.update(model_bytes=nbytes, fraction_of_8TBs=round(nbytes / (q["mean_ms"] * 1e-3) / PEAK, 3))
            other = "forward" if mode == "edge" else "composed"
            rec = dict(head, timings=timings, peak_added_bytes=peak, kernels=kernels, a_bytes=4 * E * h,
                       max_relative_difference=diff,
                       weights_over_other=round(timings["weights"]["median_ms"] / timings[other]["median_ms"], 3))
            if mode == "edge":
                fwd = kernels["forward"].get("attn_edge_fwd_rows")
                mine = kernels["weights"].get("attn_weights_xe")
                if fwd and mine:
                    rec["xe_kernel_over_forward_pass"] = round(mine["mean_ms"] / fwd["mean_ms"], 3)
            emit(rec)
            del stats, fns
        if small is not None and "edge" in args.modes.split(","):
            s4 = small.csr_args()[:4]
            Qs, Ks, Vs, xs, _ = _operands(small, h, d, args.seed, dev)
            stats = ops.attention_edge_forward(*s4, Qs, Ks, Vs, xs)[1]
            slot_row = torch.repeat_interleave(small.row, small.ptr_r[1:] - small.ptr_r[:-1])
            hh = (lambda x: x.reshape(x.size(0), h, d))

            def torch_route():
                kx = hh(Ks).index_select(0, small.indices_r) + hh(xs).index_select(0, small.eid_r)
                s_slot = (hh(Qs).index_select(0, slot_row) * kx).sum(-1)
                s = torch.zeros_like(s_slot).index_copy(0, small.eid_r, s_slot)
                return ops.sparse_softmax_forward(*s4[:3], s if h > 1 else s.reshape(-1))

            fns = {"weights": lambda: ops.attention_weights(*s4, Qs, Ks, stats, None, xs), "torch": torch_route}
            diff = _rel(fns["weights"](), torch_route())
            peak = _peaks(fns)
            timings = _summary(_timed(fns, args.warmup, args.iters))
            emit({"graph": "chung_lu_graph(%d, %d, alpha=0.5, seed=%d)" % (N, small.n_edges, args.seed),
                  "n_edges": small.n_edges, "h": h, "d": d, "mode": "edge, torch route on the cut graph",
                  "timings": timings, "peak_added_bytes": peak, "one_edge_row_tensor_bytes": 4 * small.n_edges * h * d,
                  "max_relative_difference": diff,
                  "weights_over_other": round(timings["weights"]["median_ms"] / timings["torch"]["median_ms"], 3)})
            del Qs, Ks, Vs, xs, stats, fns
        del Q, K, V, xe, b
        torch.cuda.empty_cache()
    _lib.check_errors()


if __name__ == "__main__":
    main()
