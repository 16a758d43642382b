#!/usr/bin/env python3
"""Run a randomised battery of the test suite over many more seeds than the suite does (needs an MI355X):
    python tools/soak_fuzz.py [first_seed last_seed]          # tests/test_hip_parity.py::test_fuzz_shapes_and_paths
                                                              # (shapes, heads, chunk sizes, both window orders, forced
                                                              # knobs); default 40 340
    python tools/soak_fuzz.py --gat [first_seed last_seed]    # tests/test_gat_fuzz.py::test_gat_family_fuzz (the GAT
                                                              # family, tests/gat_fuzz.py); default 48 348
    python tools/soak_fuzz.py --gat-edge [first_seed last_seed]   # tests/test_gat_edge_fuzz.py::test_gat_edge_fuzz (the
                                                              # fused GAT layer with an edge term,
                                                              # tests/gat_edge_fuzz.py); default 24 174
    python tools/soak_fuzz.py --attention [first_seed last_seed]  # tests/test_attention_fuzz.py::
                                                              # test_attention_family_fuzz (the fused dot-product
                                                              # attention family, tests/attention_fuzz.py); default 48 348
A seed that fails its assertions is counted and the run goes on.  Anything else a seed raises (a HIP error, a fault
reported by the library) stops the run at that seed with exit status 2: nothing more is started on a device that may
have faulted.  Exit status 1: some seed failed its assertions."""
import sys, os
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import torch

args = sys.argv[1:]
gat = bool(args) and args[0] in ("--gat", "--gat-edge", "--attention")
if gat and args[0] == "--attention":
    args = args[1:]
    import test_attention_fuzz as T
    run, default, cases = T.test_attention_family_fuzz, (48, 348), T.F.case_data
elif gat and args[0] == "--gat-edge":
    args = args[1:]
    import test_gat_edge_fuzz as T
    run, default, cases = T.test_gat_edge_fuzz, (24, 174), T.G.case_data
elif gat:
    args = args[1:]
    import test_gat_fuzz as T
    run, default, cases = T.test_gat_family_fuzz, (48, 348), T.F.case_data
else:
    import test_hip_parity as T
    run, default = T.test_fuzz_shapes_and_paths, (40, 340)
dev = torch.device("cuda:0")
bad = 0
lo, hi = (int(args[0]), int(args[1])) if len(args) > 1 else default
for seed in range(lo, hi):
    try:
        run(dev, seed)
    except AssertionError as e:
        bad += 1
        print("seed", seed, "FAILED", repr(e)[:600], flush=True)
    except BaseException as e:
        print("seed", seed, "RAISED", repr(e)[:600], "-- stopping, failures so far:", bad, flush=True)
        sys.exit(2)
    if gat:
        cases.cache_clear()      # (the suite keeps its cases for the host tier; a soak run need not)
    if seed % 50 == 0:
        print("seed", seed, "ok so far, failures:", bad, flush=True)
print("done, failures:", bad)
sys.exit(1 if bad else 0)
