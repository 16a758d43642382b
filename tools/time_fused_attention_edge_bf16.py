#!/usr/bin/env python3
"""Time the bfloat16 fused attention step with edge features (functions.fused_attention_edge_step on bfloat16 leaves:
FusedAttentionEdge over graphop.attention_edge_bf16_*).

Three steps alternate in one process, --warmup untimed rounds and then --repeats blocks of --iters rounds timed by device
events:
  edge_bf16   the fused edge step on bfloat16 Q / K / V / xe, xe.grad wanted;
  edge_fp32   (a) the fp32 FusedAttentionEdge of 4.5m on the same values widened, on the same build: what a bfloat16 user
              ran before, not counting the upcasts;
  plain_bf16  (b) functions.fused_attention_dropout_step on the same bfloat16 Q / K / V (the plain bf16 step of 4.5s at
              p = 0, 4.5w's at p > 0): the price of the edge term.
Reported per (h, d) and p: the median (min..max) over all timed rounds, the median of every block (the spread of repeated
runs), the per-pass kernel times of the library's launch profile for the bf16 edge step (rounds of their own) next to the
byte model of 4.5y, the largest difference of o, dQ, dK, dV, dxe against the fp32 step over the fp32 tensor's largest
value, and, at p = 0, the bf16 step against a float64 evaluation on --sample evenly spaced rows and columns (sampled_check:
the largest |got - want| / (atol + rtol |want|) at the GPU tests' bf16 bound; 1 or less is inside it).  The second check
does not lean on the fp32 op, whose generic kernels leave rows from 2^24 / h upward untouched.  Nothing is asserted.  One
process per table: one --shape per invocation.
Graph: chung_lu_graph(N of --shape, --edges (20 M, as tools/time_fused_attention_edge.py's fp32 table), alpha=0.5,
seed=--seed).  One summary record per case, printed and collected in --out (default
profiles/fused_attention_edge_bf16_bench.json; --append keeps the records there)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from custom_op_benchmark_amd import _lib, functions, graphs  # noqa: E402
from time_fused_attention_edge import _profile, _timed  # noqa: E402

RTOL, ATOL = 2 ** -8 + 1e-4, 1e-5          # BF_TOL of tests/test_attention_bf16.py


def _tensor_err(got, want):
    """max |got - want| over the largest |want| of the tensor, in pieces of 2^20 rows (xe.grad is edge-sized)"""
    diff = max(float((x.float() - y.float()).abs().max()) for x, y in zip(got.split(1 << 20), want.split(1 << 20)))
    return diff / float(want.abs().max())


def sampled_check(g, h, d, Q, K, V, xe, dO, got, n):
    """The p = 0 step in float64 on n evenly spaced rows (o, dQ, dxe: their softmax is evaluated here) and n evenly spaced
    columns (dK, dV: the weights from the op's fp32 statistics, D_i from its o) against got = (o, dQ, dK, dV, dxe, stats)."""
    f8 = lambda x: x.detach().reshape(x.size(0), h, d).double()
    o, dQ, dK, dV, dxe = (x.detach().reshape(x.size(0), h, d) for x in got[:5])
    stats = got[5].double()
    ratio = lambda x, x0: float(((x.double() - x0).abs() / (ATOL + RTOL * x0.abs())).max())
    out = {}
    rows = torch.unique(torch.linspace(0, g.n_src - 1, n, device=Q.device).long())
    pick = torch.zeros(g.n_src, dtype=torch.bool, device=Q.device)
    pick[rows] = True
    e = pick[g.src].nonzero().squeeze(1)
    src, dst = g.src[e], g.dst[e]
    kx, vx = f8(K[dst]) + f8(xe[e]), f8(V[dst]) + f8(xe[e])
    s = (f8(Q[src]) * kx).sum(-1)
    m = torch.full((g.n_src, h), float("-inf"), dtype=s.dtype, device=s.device).scatter_reduce(0, src[:, None].expand_as(s), s, "amax")
    pe = torch.exp(s - m[src])
    a = pe / torch.zeros_like(m).index_add_(0, src, pe)[src]
    D = (f8(dO) * o.double()).sum(-1)
    ds = a * ((f8(dO[src]) * vx).sum(-1) - D[src])
    zq = torch.zeros((g.n_src, h, d), dtype=s.dtype, device=s.device)
    out["o"] = ratio(o[rows], zq.clone().index_add_(0, src, a[..., None] * vx)[rows])
    out["dQ"] = ratio(dQ[rows], zq.clone().index_add_(0, src, ds[..., None] * kx)[rows])
    out["dxe"] = ratio(dxe[e], ds[..., None] * f8(Q[src]) + a[..., None] * f8(dO[src]))
    out["rows"], out["row_edges"], out["largest_row"] = int(rows.numel()), int(e.numel()), int(rows.max())
    del kx, vx, s, m, pe, a, ds, zq
    cols = torch.unique(torch.linspace(0, g.n_dst - 1, n, device=Q.device).long())
    pick = torch.zeros(g.n_dst, dtype=torch.bool, device=Q.device)
    pick[cols] = True
    e = pick[g.dst].nonzero().squeeze(1)
    src, dst = g.src[e], g.dst[e]
    xs = f8(xe[e])
    a = torch.exp((f8(Q[src]) * (f8(K[dst]) + xs)).sum(-1) - stats[src, :, 0]) * stats[src, :, 1]
    ds = a * ((f8(dO[src]) * (f8(V[dst]) + xs)).sum(-1) - D[src])
    zk = torch.zeros((g.n_dst, h, d), dtype=a.dtype, device=a.device)
    out["dK"] = ratio(dK[cols], zk.clone().index_add_(0, dst, ds[..., None] * f8(Q[src]))[cols])
    out["dV"] = ratio(dV[cols], zk.clone().index_add_(0, dst, a[..., None] * f8(dO[src]))[cols])
    out["cols"], out["col_edges"] = int(cols.numel()), int(e.numel())
    return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in out.items()}


def byte_model(E, F, h, identity_r):
    """bytes per pass that grow with E (4.5y): ids, the gathers and the edge row, bf16 against fp32"""
    ids_r, ids_c = 8 + (0 if identity_r else 8), 16          # int64 neighbour id (+ int64 edge id) per slot
    per = lambda es: {"fwd_rows": E * (ids_r + 2 * es * F + es * F), "rows_row": E * (ids_r + 2 * es * F + 2 * es * F),
                      "rows_col": E * (ids_c + 2 * es * F + es * F + 16 * h)}
    return {"bf16": per(2), "fp32": per(4)}


def _lib_stats(g, Q, K, V, xe):
    """the fp32 statistics the bf16 forward leaves (the autograd class keeps them to itself)"""
    from custom_op_benchmark_amd import graphop
    return graphop.attention_edge_bf16_forward(*g.csr_args()[:4], Q.detach(), K.detach(), V.detach(), xe.detach())[1]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", default="reddit", choices=sorted(graphs.SHAPES))
    ap.add_argument("--edges", type=int, default=20_000_000, metavar="N", help="N edges instead of the default 20 M")
    ap.add_argument("--hd", default="1x64,4x64,8x32,8x64", help="comma-separated h x d pairs")
    ap.add_argument("--dropout", default="0,0.5", help="comma-separated dropout probabilities")
    ap.add_argument("--dropout-seed", type=int, default=1234567890123)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=2, help="blocks of --iters rounds; their medians show the run-to-run spread")
    ap.add_argument("--sample", type=int, default=512, help="rows and columns of the float64 check at p = 0")
    ap.add_argument("--chunk-size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--append", action="store_true", help="keep the records --out already holds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_attention_edge_bf16_bench.json"))
    args = ap.parse_args()
    dev, bf = torch.device("cuda:0"), torch.bfloat16
    N, _ = graphs.SHAPES[args.shape]
    g = graphs.chung_lu_graph(N, args.edges, alpha=0.5, seed=args.seed, chunk_size=args.chunk_size, device=dev)
    E, n_q, n_k = g.n_edges, g.n_src, g.n_dst
    identity_r = bool(torch.equal(g.eid_r, torch.arange(E, device=g.eid_r.device)))
    records = []
    if args.append and os.path.exists(args.out):
        with open(args.out) as fh:
            records = json.load(fh)
    for hd in args.hd.split(","):
        h, d = (int(x) for x in hd.split("x"))
        gen = torch.Generator(device=dev).manual_seed(args.seed + h * 100 + d)
        ns = (lambda n: (n, d) if h == 1 else (n, h, d))
        Q = (torch.randn(ns(n_q), generator=gen, device=dev) / d ** 0.5).to(bf).requires_grad_(True)
        K = torch.randn(ns(n_k), generator=gen, device=dev).to(bf).requires_grad_(True)
        V = torch.randn(ns(n_k), generator=gen, device=dev).to(bf).requires_grad_(True)
        dO = (torch.randn(ns(n_q), generator=gen, device=dev) / d ** 0.5).to(bf)
        xe = torch.randn(ns(E), generator=gen, device=dev).to(bf).requires_grad_(True)
        Qf, Kf, Vf, xef = (x.detach().float().requires_grad_(True) for x in (Q, K, V, xe))
        dOf = dO.float()
        leaves = (Q, K, V, xe, Qf, Kf, Vf, xef)

        def clear():
            for x in leaves:
                x.grad = None

        for p in (float(x) for x in args.dropout.split(",")):
            drop = (p, args.dropout_seed, 7)

            def edge_bf16():
                clear()
                return functions.fused_attention_edge_step(g, Q, K, V, xe, dO, *drop)

            def edge_fp32():
                clear()
                return functions.fused_attention_edge_step(g, Qf, Kf, Vf, xef, dOf, *drop)

            def plain_bf16():
                clear()
                return functions.fused_attention_dropout_step(g, Q, K, V, dO, *drop)

            fns = {"edge_bf16": edge_bf16, "edge_fp32": edge_fp32, "plain_bf16": plain_bf16}
            got = {}
            for name in ("edge_bf16", "edge_fp32"):          # plans and caches; the results of one call each
                o = fns[name]().detach()
                torch.cuda.synchronize()
                got[name] = [o] + [x.grad for x in (leaves[4:] if name == "edge_fp32" else leaves[:4])]
            err = {n: _tensor_err(x, y) for n, x, y in zip(("o", "dQ", "dK", "dV", "dxe"), got["edge_bf16"], got["edge_fp32"])}
            sampled = None
            if p == 0.0:          # (the sampled check states no multipliers)
                stats = _lib_stats(g, Q, K, V, xe)
                sampled = sampled_check(g, h, d, Q, K, V, xe, dO, got["edge_bf16"] + [stats], args.sample)
                del stats
            del got, o
            clear()
            blocks = [_timed(fns, args.warmup if r == 0 else 0, args.iters) for r in range(args.repeats)]
            timings = {}
            for n in fns:
                v = [x for b in blocks for x in b[n]]
                timings[n] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                              "block_medians_ms": [round(statistics.median(b[n]), 4) for b in blocks]}
            kernels = {tag: {"kernel": q["kernel"], "calls": q["calls"], "mean_ms": round(q["mean_ms"], 4),
                             "min_ms": round(q["min_ms"], 4)}
                       for tag, q in sorted(_profile(edge_bf16, args.iters).items()) if tag.startswith("attn_edge_bf16")}
            kernels_fp32 = {tag: {"kernel": q["kernel"], "calls": q["calls"], "mean_ms": round(q["mean_ms"], 4),
                                  "min_ms": round(q["min_ms"], 4)}
                            for tag, q in sorted(_profile(edge_fp32, args.iters).items()) if tag.startswith("attn_edge_")}
            a = timings["edge_bf16"]["median_ms"]
            ratios = lambda n: [round(x / y, 3) for x, y in zip(timings["edge_bf16"]["block_medians_ms"],
                                                                 timings[n]["block_medians_ms"])]
            rec = {"tool": "tools/time_fused_attention_edge_bf16.py",
                   "graph": "chung_lu_graph(%d, %d, alpha=0.5, seed=%d)" % (N, E, args.seed), "shape": args.shape,
                   "n_q": n_q, "n_k": n_k, "n_edges": E, "row_chunks": g.n_row_chunks, "col_chunks": g.n_col_chunks,
                   "chunk_size": args.chunk_size, "eid_identity_row_major": identity_r, "h": h, "d": d,
                   "dropout": {"p": drop[0], "seed": drop[1], "offset": drop[2]}, "warmup": args.warmup,
                   "iters": args.iters, "repeats": args.repeats, "difference_vs_fp32_step_over_its_largest_value": err,
                   "sampled_float64_check_ratio_of_bf16_bound": sampled,
                   "timings": timings,
                   "edge_bf16_over_edge_fp32": round(a / timings["edge_fp32"]["median_ms"], 3),
                   "edge_bf16_over_edge_fp32_by_block": ratios("edge_fp32"),
                   "edge_bf16_over_plain_bf16": round(a / timings["plain_bf16"]["median_ms"], 3),
                   "edge_bf16_over_plain_bf16_by_block": ratios("plain_bf16"),
                   "byte_model": byte_model(E, h * d, h, identity_r), "kernels": kernels, "kernels_fp32": kernels_fp32,
                   "device": torch.cuda.get_device_name(dev)}
            print(json.dumps(rec), flush=True)
            records.append(rec)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:      # rewritten after every case: a run that is cut short keeps what it has
                fh.write("[\n" + ",\n".join(json.dumps(r) for r in records) + "\n]\n")          # one line per record
        del Q, K, V, dO, xe, Qf, Kf, Vf, xef, dOf, leaves
        torch.cuda.empty_cache()
    _lib.check_errors()


if __name__ == "__main__":
    main()
