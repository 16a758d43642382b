"""CPU tier: the C-ABI library loads and exports every symbol include/graphop_hip.h declares;
the Python host mirrors the reference surface and its error behaviour.  No compute calls."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "graphop_hip.h")).read()
    return sorted(set(re.findall(r"GRAPHOP_API\s+[\w\s\*]+?\b(graphop_\w+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from custom_op_benchmark_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    syms = _header_symbols()
    assert len(syms) >= 15
    l = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(l, s), "missing export " + s
    assert sorted(_lib.EXPORTED_SYMBOLS) == syms          # binding covers the whole header
    assert _lib.lib().graphop_abi_version() == _lib.ABI_VERSION


def test_argument_validation_without_gpu():
    """Entry points reject bad sizes / dtypes before touching the device."""
    from custom_op_benchmark_amd import _lib
    l = _lib.lib()
    n = ctypes.c_void_p(0)
    rc = l.graphop_maskedmm_csr_forward(7, n, n, n, n, n, n, n, 0, 0, 0, 0, 1, 4, n, n)
    assert rc == 1 and b"dtype" in l.graphop_last_error()
    rc = l.graphop_vector_spmm_forward(0, n, n, n, n, n, n, n, -1, 0, 0, 0, 1, 4, n, n)
    assert rc == 1 and b"negative" in l.graphop_last_error()
    rc = l.graphop_partition_csr_count(n, 0, 32, n, n)
    assert rc == 1
    # empty problems are no-ops that never dereference anything
    assert l.graphop_maskedmm_csr_forward(0, n, n, n, n, n, n, n, 0, 0, 0, 0, 1, 4, n, n) == 0
    assert l.graphop_sparse_softmax_forward(0, n, n, n, n, n, 0, 0, 1, n, 0, n, n) == 0


def test_module_surface_matches_reference():
    import graphop
    from custom_op_benchmark_amd import functions
    names = ["maskedmm_csr_forward", "maskedmm_csr_backward", "node_mul_edge_forward",
             "node_mul_edge_backward", "sparse_softmax_forward", "sparse_softmax_backward",
             "vector_spmm_forward", "vector_spmm_backward"]          # graphop.cpp:217-224
    assert sorted(graphop.__all__) == sorted(names)
    for n in names:
        assert callable(getattr(graphop, n))
        assert hasattr(torch.ops.graphop, n)
    for cls in ("SparseSoftmax", "MaskedMMCSR", "NodeMulEdge", "VectorSPMM"):   # wrapper.py:8-55
        assert issubclass(getattr(functions, cls), torch.autograd.Function)


def test_cpu_tensors_are_refused_like_the_reference():
    """CHECK_CUDA (graphop.cpp:4): '<arg> must be a CUDA tensor'.  No silent CPU fallback."""
    import graphop
    i = torch.zeros(2, dtype=torch.int64)
    f = torch.zeros(2, 4)
    with pytest.raises(RuntimeError, match="row must be a CUDA tensor"):
        graphop.maskedmm_csr_forward(i, i, i, i, f, f)
    with pytest.raises(RuntimeError, match="row must be a CUDA tensor"):
        graphop.sparse_softmax_forward(i, i, i, f[:, 0].contiguous())
    with pytest.raises(RuntimeError, match="row must be a CUDA tensor"):
        graphop.vector_spmm_backward(i, i, i, i, i, i, i, i, f, f, f)
    with pytest.raises(RuntimeError, match="no CPU implementation|must be a CUDA tensor"):
        torch.ops.graphop.sparse_softmax_forward(i, i, i, f[:, 0].contiguous())


def test_missing_library_fails_loudly(monkeypatch):
    from custom_op_benchmark_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libgraphop_hip.so")
    with pytest.raises(RuntimeError, match="has not been built"):
        _lib.lib()


def test_product_never_imports_oracle():
    """The product package must not reference the oracle (test infrastructure)."""
    pkg = os.path.join(ROOT, "custom_op_benchmark_amd")
    for base, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(base, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, re.M), f
                assert "liboracle" not in txt and "graphop_oracle" not in txt, f


def test_graph_container_roundtrip(tmp_path):
    from custom_op_benchmark_amd import graphs
    g = graphs.uniform_random_graph(50, 700, seed=1, chunk_size=8)
    p = str(tmp_path / "g.pt")
    graphs.save_graph(g, p)
    g2 = graphs.load_graph(p)
    for k, v in g.__dict__.items():
        w = getattr(g2, k)
        assert torch.equal(v, w) if isinstance(v, torch.Tensor) else v == w


def test_block_diagonal_graph_matches_reference_formula():
    """eid_c[cnt] = b*l*l + (x % l)*l + (y % l) for column-major slot (b, y, x)  (wrapper.py:104-112)."""
    from custom_op_benchmark_amd import graphs
    bs, l = 4, 5
    g = graphs.block_diagonal_graph(bs, l, chunk_size=3)
    eid_c, indices_c, indptr_c = [], [], []
    cnt = 0
    for b in range(bs):
        for y in range(b * l, (b + 1) * l):
            indptr_c.append(cnt)
            for x in range(b * l, (b + 1) * l):
                indices_c.append(x); eid_c.append(b * l * l + (x % l) * l + (y % l)); cnt += 1
    indptr_c.append(cnt)
    assert g.eid_c.tolist() == eid_c and g.indices_c.tolist() == indices_c and g.indptr_c.tolist() == indptr_c
    assert g.eid_r.tolist() == list(range(bs * l * l))


def test_hot_kernels_do_not_spill():
    """Register budget of the shipped code object: no window-owner / block-dense / softmax-segment /
    fused-attention kernel may spill VGPRs or use scratch (each is compiled for a stated number of
    resident workgroups per CU, kernels_fast.h: sweep_bpc; a spill in their inner loops costs more
    than the occupancy it buys).  Read from the AMDGPU metadata note of libgraphop_hip.so."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources()
    hot = {n: r for n, r in res.items()
           if re.search(r"k_(sddmm|spmm)_(wown|block|wown_staged|walk)_f(32|64)|k_softmax_(fwd|bwd)_(seg|vec4)|k_attn_bwd_wown_f32|k_nme_", n)}
    assert len(hot) > 100, len(hot)
    bad = {n: r for n, r in hot.items() if r["spill_vgpr"] or r["scratch"]}
    assert not bad, "\n".join("%s: %r" % kv for kv in sorted(bad.items()))
    # the headline instantiations keep 4 workgroups per CU (<= 128 VGPRs); the fused passes with staged
    # ids are compiled for 3 (<= 168)
    for n, r in hot.items():
        if re.search(r"k_(sddmm|spmm)_wown(_staged)?_f32<16, 1, true", n) or re.search(r"k_attn_bwd_wown_f32<16, 1, false, (true|false), 4, false>", n):
            assert r["vgpr"] <= 128, (n, r)
        if re.search(r"k_attn_bwd_wown_f32<16, 1, (true|false), (true|false), 3, true>", n):
            assert r["vgpr"] <= 168, (n, r)


def test_dlpack_interchange_cpu():
    """README.md:5-7 TODO of the reference ("Switch backend to dlpack"): the eight index arrays travel
    as DLPack capsules / from any __dlpack__ producer, zero-copy."""
    import numpy as np
    from custom_op_benchmark_amd import graphs
    g = graphs.uniform_random_graph(40, 500, seed=3, chunk_size=8, n_dst=55)
    caps = graphs.to_dlpack(g)
    assert set(caps) == {"row", "ptr_r", "eid_r", "indices_r", "col", "ptr_c", "eid_c", "indices_c"}
    g2 = graphs.from_dlpack(caps, g.n_src, g.n_dst, chunk_size=8)
    for k in ("row", "ptr_r", "eid_r", "indices_r", "col", "ptr_c", "eid_c", "indices_c", "indptr_r", "indptr_c", "src", "dst"):
        assert torch.equal(getattr(g, k), getattr(g2, k)), k
    assert g2.indices_r.data_ptr() == g.indices_r.data_ptr()        # zero-copy
    # a foreign producer: numpy arrays implement __dlpack__
    arrs = {k: np.asarray(getattr(g, k)) for k in caps}
    g3 = graphs.from_dlpack(arrs, g.n_src, g.n_dst, chunk_size=8)
    assert torch.equal(g3.indptr_c, g.indptr_c) and torch.equal(g3.eid_c, g.eid_c)
    with pytest.raises(RuntimeError, match="int64"):
        bad = dict(arrs); bad["row"] = arrs["row"].astype(np.int32)
        graphs.from_dlpack(bad, g.n_src, g.n_dst)


def test_container_reads_format_1(tmp_path):
    """Round-1 containers (no plan state) still load."""
    from custom_op_benchmark_amd import graphs
    g = graphs.uniform_random_graph(30, 200, seed=5, chunk_size=8)
    payload = {"format": 1}
    payload.update({k: v for k, v in g.__dict__.items()})
    p = str(tmp_path / "old.pt")
    torch.save(payload, p)
    assert torch.equal(graphs.load_graph(p).eid_c, g.eid_c)


def test_cpp_extension_mirrors_the_reference_module():
    """csrc/torch_ext.cpp, built by __graft_entry__.build(): a compiled PyTorch C++ extension with the
    reference's eight pybind11 functions (graphop.cpp:216-225) AND TORCH_LIBRARY(graphop); CHECK_CUDA /
    CHECK_CONTIGUOUS raise the reference's messages (graphop.cpp:4-6) before anything touches a device."""
    from custom_op_benchmark_amd import _ext, graphop
    ext = _ext.load()
    if ext is None:
        pytest.skip("graphop_cpp.so not built (run __graft_entry__.build())")
    names = ["maskedmm_csr_forward", "maskedmm_csr_backward", "node_mul_edge_forward", "node_mul_edge_backward",
             "sparse_softmax_forward", "sparse_softmax_backward", "vector_spmm_forward", "vector_spmm_backward"]
    for n in names + ["attention_forward", "attention_backward"]:
        assert callable(getattr(ext, n)) and hasattr(torch.ops.graphop, n)
    assert graphop.cpp_ext is ext                      # torch.ops.graphop.* was registered from C++
    i = torch.zeros(2, dtype=torch.int64)
    f = torch.zeros(2, 4)
    with pytest.raises(RuntimeError, match="row must be a CUDA tensor"):
        ext.maskedmm_csr_forward(i, i, i, i, f, f)
    with pytest.raises(RuntimeError, match="row must be a CUDA tensor"):
        ext.vector_spmm_backward(i, i, i, i, i, i, i, i, f, f, f)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        torch.ops.graphop.attention_forward(i, i, i, i, f, f, f)
    with pytest.raises(TypeError):
        ext.sparse_softmax_forward(i, i, i)            # positional signature, 4 arguments (graphop.cpp:59-63)


def test_registered_schemas_equal_the_python_table():
    """torch_ext.cpp's op table and graphop.py's _SCHEMAS state the same ops with the same schemas.  Parsed schemas are
    compared, not text: a registered `float p=0.0` prints as `0.`, `ScalarType dtype=float` as `6`."""
    from custom_op_benchmark_amd import graphop as ops
    assert ops.cpp_ext is not None, "graphop_cpp.so not built (run __graft_entry__.build())"
    for n, schema in ops._SCHEMAS.items():
        assert torch._C.parse_schema("graphop::" + n + schema) == getattr(torch.ops.graphop, n).default._schema, n
    registered = {s.name.split("::")[1] for s in torch._C._jit_get_all_schemas() if s.name.startswith("graphop::")}
    assert registered == set(ops._SCHEMAS)


def test_pybind_keywords_follow_the_schemas():
    """The pybind list of torch_ext.cpp is written by hand: where it names its arguments, their names, which of them
    have defaults and the int / float / bool default values are the schema's.  The reference's eight and attention_* take
    positional arguments only, like the reference's module."""
    import ast
    from custom_op_benchmark_amd import graphop as ops
    assert ops.cpp_ext is not None, "graphop_cpp.so not built (run __graft_entry__.build())"
    positional = set(ops.__all__) | {"attention_forward", "attention_backward"}
    assert len(positional) == 10
    for n in ops._SCHEMAS:
        want = getattr(torch.ops.graphop, n).default._schema.arguments
        sig = getattr(ops.cpp_ext, n).__doc__.splitlines()[0]
        assert sig.startswith(n + "(") and ") -> " in sig, sig
        params = sig[len(n) + 1:sig.rindex(") -> ")].split(", ")
        assert len(params) == len(want), sig
        if n in positional:
            assert [p.split(":")[0] for p in params] == ["arg%d" % k for k in range(len(want))], sig
            continue
        for p, a in zip(params, want):
            name, _, rest = p.partition(": ")
            _, eq, default = rest.partition(" = ")
            assert name == a.name and bool(eq) == a.has_default_value(), (n, p)
            if eq:
                try:
                    value = ast.literal_eval(default)
                except ValueError:          # `torch.float32`: no int / float / bool
                    assert a.name == "dtype", (n, p)
                    continue
                assert type(value) is type(a.default_value) and value == a.default_value, (n, p)


def test_head_group_rule_and_labelings():
    """Host logic of round 5: FusedAttention's head-group size (256-B rows, one head per group from d = 64 on, blocking only
    where it saves memory) and the generator's node labelings (bench.py --labeling)."""
    import torch
    from custom_op_benchmark_amd import functions, graphs
    hg = functions._head_group
    assert [hg(8, 32), hg(8, 16), hg(8, 64), hg(8, 128), hg(2, 32), hg(6, 16), hg(3, 16)] == [2, 4, 1, 1, 2, 3, 3]
    assert all(hg(h, d) * d * 4 <= 256 or hg(h, d) == 1 for h in (2, 4, 8, 16) for d in (8, 16, 32, 64, 128))
    assert hg(8, 32, 114_615_892, 232_965) == 2          # Reddit shape: edge tensors dominate -> groups
    assert hg(8, 16, 61_859_140, 2_449_029) == 8         # products shape: node tensors dominate -> no blocking
    n, e = 4000, 160_000
    deg = {}
    for lab in graphs.LABELINGS:
        g = graphs.chung_lu_graph(n, e, alpha=0.5, seed=1, labeling=lab, community=100)
        assert g.n_edges == e and int(g.indices_r.max()) < n
        deg[lab] = (g.indptr_c[1:] - g.indptr_c[:-1]).float()
        same = ((g.src // 100) == (g.dst // 100)).float().mean()
        assert (same > 0.85) == (lab == "clustered"), (lab, float(same))
    # ids sorted by degree: the first tenth of the ids holds far more than a tenth of the slots; shuffled: about a tenth
    assert float(deg["degree"][: n // 10].sum()) > 0.25 * e and abs(float(deg["shuffled"][: n // 10].sum()) / e - 0.1) < 0.03
    with __import__("pytest").raises(ValueError):
        graphs.chung_lu_graph(10, 10, labeling="nope")
